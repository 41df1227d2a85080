/*
 * iso_harness.cpp -- host build (g++) of the per-ray code of an isosurface frame (libre_amd/csrc/vrc_core.h: vrc_pixel_mip
 * with VRC_FOLD_FIRST), for tests/test_iso_cpu.py.  TEST INFRASTRUCTURE ONLY: depth_harness.cpp next to it with the
 * first-crossing fold, the running gradient per pixel, and the isovalue and ambient share of vrc_set_isosurface.
 *
 * A row-major atlas of uint8, uint16 or float voxels goes into the micro-blocked layout; the per-slot words the brick
 * upload leaves on the GPU (uniformity, largest and smallest stored value) are reduced here over each slot's brick, and
 * the frame is marched by the instances the launchers of vrc_kernels_mip.h pick.
 */
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vrc_hip.h"
#include "../../libre_amd/csrc/vrc_tables.h"

namespace
{
template < typename T >
void upload( const void* rowMajor, const uint32_t atlasDim[3], const vrc_layout& lay, const uint32_t brick[3],
             std::vector< T >& atlas, std::vector< uint32_t >& info, std::vector< uint32_t >& top,
             std::vector< uint32_t >& low )
{
    const T* const src = static_cast< const T* >( rowMajor );
    atlas.resize( (size_t)atlasDim[0] * atlasDim[1] * atlasDim[2] );
    const uint32_t nSlots = lay.slots[0] * lay.slots[1] * lay.slots[2];
    info.assign( nSlots, 0u );
    top.assign( nSlots, 0u );
    low.assign( nSlots, 0u );
    std::vector< T > first( nSlots );
    for( uint32_t z = 0; z < atlasDim[2]; ++z )
        for( uint32_t y = 0; y < atlasDim[1]; ++y )
            for( uint32_t x = 0; x < atlasDim[0]; ++x )
            {
                const T v = src[( (size_t)z * atlasDim[1] + y ) * atlasDim[0] + x];
                atlas[vrc_atlas_index( lay, x, y, z )] = v;
                const uint32_t i = x / lay.slotDim[0], j = y / lay.slotDim[1], k = z / lay.slotDim[2];
                const uint32_t lx = x - i * lay.slotDim[0], ly = y - j * lay.slotDim[1], lz = z - k * lay.slotDim[2];
                if( lx >= brick[0] || ly >= brick[1] || lz >= brick[2] )
                    continue; /* slot padding: the upload repeats voxels of the brick there */
                const uint32_t slot = ( k * lay.slots[1] + j ) * lay.slots[0] + i;
                uint32_t key, keyMin;
                if constexpr( sizeof( T ) == 4 )
                {
                    float fv;
                    std::memcpy( &fv, &v, 4 );
                    key = fv != fv ? vrc_slot_max_key( -INFINITY ) : vrc_slot_max_key( fv );
                    keyMin = fv != fv ? vrc_slot_min_key( INFINITY ) : vrc_slot_min_key( fv );
                }
                else
                {
                    key = (uint32_t)v + 1u;
                    keyMin = vrc_slot_min_key( (uint32_t)v );
                }
                top[slot] = key > top[slot] ? key : top[slot];
                low[slot] = keyMin > low[slot] ? keyMin : low[slot];
                if constexpr( sizeof( T ) <= 2 )
                {
                    if( !( info[slot] & VRC_SLOT_KNOWN ) )
                    {
                        first[slot] = v;
                        info[slot] = VRC_SLOT_KNOWN | (uint32_t)v;
                    }
                    else if( v != first[slot] )
                        info[slot] |= VRC_SLOT_MIXED;
                }
            }
}
} // namespace

/* mipMax, mipDepth, isoGrad: W x H (x 3) running V bits, D and G of the passes (first != 0: not read).  iso, ambient:
 * vrc_set_isosurface's (the scenes here hold unsigned voxels: no shift).  interval: W x H x 8 or null, every ray as
 * vrc_setup_ray leaves it: tNearGlobal, tFarGlobal, origin and direction.
 * form: bit 0 = grid walk (else reference order), bit 1 = fixed-point stepping, bit 3 = trilinear samples, bit 4 =
 * skipping (VRC_OPT_MIP_SKIP), bit 5 = uniform bricks.  voxelBytes: 1, 2 or 4 (float).  perPixel: W x H sample counts of
 * this call, or null.  values, counts: W x H entries, what vrc_get_projection_values returns after this pass. */
extern "C" int iso_harness_render( const void* atlasRowMajor, uint32_t voxelBytes, const uint32_t atlasDim[3],
                                  const uint32_t slotDim[3], const uint32_t brickDim[3], float* pixelBuffer,
                                  uint32_t* mipMax, float* mipDepth, float* isoGrad, float iso, float ambient,
                                  float* interval, uint32_t W, uint32_t H, const float* planes, uint32_t nPlanes,
                                  const float* tf, const vrc_view_data* view, uint32_t nNodes, const vrc_node_data* nodes,
                                  const vrc_render_data* render, int form, int fracBits, int first,
                                  uint64_t* samplesOut, uint32_t* perPixel, float* values, uint32_t* counts )
{
    if( iso != iso || !( ambient >= 0.0f && ambient <= 1.0f ) )
        return 1;
    vrc_atlas_geom geom;
    vrc_layout lay;
    for( int a = 0; a < 3; ++a )
    {
        if( atlasDim[a] % 8u || slotDim[a] % 8u || atlasDim[a] % slotDim[a] )
            return 1;
        geom.atlasDim[a] = atlasDim[a];
        geom.slotDim[a] = slotDim[a];
        geom.slots[a] = lay.slots[a] = atlasDim[a] / slotDim[a];
        lay.slotDim[a] = slotDim[a];
    }
    std::vector< uint8_t > atlas8;
    std::vector< uint16_t > atlas16;
    std::vector< uint32_t > atlas32, info, top, low;
    if( voxelBytes == 1 )
        upload< uint8_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas8, info, top, low );
    else if( voxelBytes == 2 )
        upload< uint16_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas16, info, top, low );
    else if( voxelBytes == 4 )
        upload< uint32_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas32, info, top, low );
    else
        return 1;
    const float* const atlasF = reinterpret_cast< const float* >( atlas32.data() );

    vrc_lut_params lp;
    lp.rangeMin = render->dataSourceRange[0];
    lp.rangeMax = render->dataSourceRange[1];
    lp.alphaCorrection = 1.0f;
    lp.fracBits = fracBits;
    const vrc_classifier cls = vrc_make_classifier( lp );
    std::vector< vrc_f4 > tfp( VRC_TFP_ENTRIES );
    for( uint32_t k = 0; k < VRC_TFP_ENTRIES; ++k )
    {
        const uint32_t i = k == 0 ? 0u : ( k - 1u > 255u ? 255u : k - 1u );
        tfp[k] = vrc_f4{ tf[i * 4], tf[i * 4 + 1], tf[i * 4 + 2], tf[i * 4 + 3] };
    }
    vrc_host_tables t;
    vrc_build_tables( geom, nodes, nNodes, t );
    const bool grid = ( form & 1 ) != 0, linear = ( form & 8 ) != 0;
    if( grid && !t.gridOk )
        return 2;
    const bool fixed = ( form & 2 ) != 0 && !linear && !t.clamp && slotDim[0] <= 248u && slotDim[1] <= 248u && slotDim[2] <= 248u;
    float pl[6][4];
    std::memset( pl, 0, sizeof( pl ) );
    for( uint32_t i = 0; i < nPlanes && i < 6; ++i )
        for( int k = 0; k < 4; ++k )
            pl[i][k] = planes[i * 4 + k];
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    vrc_fill_frame( f, *view, *render, geom, t.g, pl, nPlanes, nNodes, W, H, 0.f, 0.f );
    f.variant = VRC_VARIANT_CUDA;
    f.clearFirst = first ? 1u : 0u;
    f.mipFirst = first ? 1u : 0u;
    f.mipMax = mipMax;
    f.slotMax = ( form & 16 ) ? top.data() : nullptr;
    f.mipDepth = mipDepth;
    f.isoGrad = isoGrad;
    f.isoThreshold = vrc_iso_int_threshold( iso, 0.0f, voxelBytes == 1 ? 255u : 65535u );
    f.isoStored = vrc_iso_float_threshold( iso, 0.0f );
    f.isoClassify = iso;
    f.isoAmbient = ambient;
    f.slotInfo = ( form & 32 ) ? info.data() : nullptr;

    uint64_t total = 0;
    vrc_f4* pb = reinterpret_cast< vrc_f4* >( pixelBuffer );
    for( uint32_t py = 0; py < H; ++py )
        for( uint32_t px = 0; px < W; ++px )
        {
            uint32_t n = 0;
#define ARGS( A ) f, t.nodes.data(), t.grid.data(), A, tfp.data(), cls, pb, px, py, n
#define FORMS( MODE, FIXED, T, A )                                                          \
    {                                                                                       \
        if( grid && t.clamp ) vrc_pixel_mip< true, true, false, MODE, T >( ARGS( A ) );     \
        else if( grid ) vrc_pixel_mip< true, false, FIXED, MODE, T >( ARGS( A ) );          \
        else if( t.clamp ) vrc_pixel_mip< false, true, false, MODE, T >( ARGS( A ) );       \
        else vrc_pixel_mip< false, false, FIXED, MODE, T >( ARGS( A ) );                    \
    }
#define TYPED( T, A )                                                                                          \
    {                                                                                                          \
        if( linear ) FORMS( VRC_MODE_WITH_FOLD( VRC_MODE_MIP_TRILINEAR, VRC_FOLD_FIRST ), false, T, A )        \
        else if( fixed ) FORMS( VRC_MODE_WITH_FOLD( VRC_MODE_MIP, VRC_FOLD_FIRST ), true, T, A )               \
        else FORMS( VRC_MODE_WITH_FOLD( VRC_MODE_MIP, VRC_FOLD_FIRST ), false, T, A )                          \
    }
            if( voxelBytes == 4 ) TYPED( float, atlasF )
            else if( voxelBytes == 2 ) TYPED( uint16_t, atlas16.data() )
            else TYPED( uint8_t, atlas8.data() )
#undef TYPED
#undef FORMS
#undef ARGS
            total += n;
            if( perPixel )
                perPixel[(size_t)py * W + px] = n;
            const size_t i = (size_t)py * W + px;
            if( values && counts )
                vrc_projection_value( (uint32_t)VRC_FOLD_FIRST, linear || voxelBytes == 4, 0.0f, mipMax[i], 0ull, 0u, values[i], counts[i] );
            if( interval )
            {
                const vrc_ray r = vrc_setup_ray( f, px, py );
                float* const o = interval + 8 * i;
                o[0] = r.tNearGlobal;
                o[1] = r.tFarGlobal;
                o[2] = r.origin.x, o[3] = r.origin.y, o[4] = r.origin.z;
                o[5] = r.dir.x, o[6] = r.dir.y, o[7] = r.dir.z;
            }
        }
    if( samplesOut )
        *samplesOut = total;
    return 0;
}

/* the two thresholds a frame is marched with (vrc_core.h), for tests/test_iso_cpu.py */
extern "C" uint32_t iso_harness_int_threshold( float iso, float shift, uint32_t typeMax )
{
    return vrc_iso_int_threshold( iso, shift, typeMax );
}
extern "C" float iso_harness_float_threshold( float iso, float shift )
{
    return vrc_iso_float_threshold( iso, shift );
}
