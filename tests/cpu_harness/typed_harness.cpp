/*
 * typed_harness.cpp -- host build (g++) of the per-ray code of libre_amd/csrc/vrc_core.h over the atlases of
 * vrc_pool_create_typed (include/vrc_hip.h), for tests/test_voxel_types_cpu.py.  TEST INFRASTRUCTURE ONLY, like
 * harness.cpp next to it.
 *
 * A row-major atlas of any of the seven voxel types goes through what the brick upload does to it on the GPU
 * (vrc_voxel_xform: the sign flip of int8 / int16, the conversion of uint32 / int32 to float32) into the micro-blocked
 * layout, and is marched by the instances the launchers of vrc_kernels.hip pick for it: ATLAS_T = float for the 4-byte
 * types (VRC_MODE_POINT, VRC_MODE_POINT_GREY, VRC_MODE_TRILINEAR), the 8- and 16-bit instances with dataSourceRange
 * moved by 128 / 32768 for the signed types.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vrc_hip.h"
#include "../../libre_amd/csrc/vrc_tables.h"

namespace
{
/* voxel type -> bytes, upload transform, range shift: the table of pool_create (vrc_api.hip) */
bool type_traits_of( int voxelType, uint32_t& bytes, int& xform, float& shift )
{
    xform = VRC_XF_NONE;
    shift = 0.0f;
    switch( voxelType )
    {
    case VRC_VOXEL_UINT8: bytes = 1; return true;
    case VRC_VOXEL_UINT16: bytes = 2; return true;
    case VRC_VOXEL_INT8: bytes = 1; xform = VRC_XF_FLIP; shift = 128.0f; return true;
    case VRC_VOXEL_INT16: bytes = 2; xform = VRC_XF_FLIP; shift = 32768.0f; return true;
    case VRC_VOXEL_UINT32: bytes = 4; xform = VRC_XF_U32F; return true;
    case VRC_VOXEL_INT32: bytes = 4; xform = VRC_XF_I32F; return true;
    case VRC_VOXEL_FLOAT32: bytes = 4; return true;
    default: return false;
    }
}

template < typename T >
T xform_voxel( int xform, T v )
{
    if constexpr( sizeof( T ) == 4 )
        return xform == VRC_XF_U32F   ? vrc_voxel_xform< VRC_XF_U32F, T >( v )
               : xform == VRC_XF_I32F ? vrc_voxel_xform< VRC_XF_I32F, T >( v )
                                      : v;
    else
        return xform == VRC_XF_FLIP ? vrc_voxel_xform< VRC_XF_FLIP, T >( v ) : v;
}

template < typename T >
void upload( const void* rowMajor, const uint32_t atlasDim[3], const vrc_layout& lay, int xform, std::vector< T >& atlas )
{
    const T* const src = static_cast< const T* >( rowMajor );
    atlas.resize( (size_t)atlasDim[0] * atlasDim[1] * atlasDim[2] );
    for( uint32_t z = 0; z < atlasDim[2]; ++z )
        for( uint32_t y = 0; y < atlasDim[1]; ++y )
            for( uint32_t x = 0; x < atlasDim[0]; ++x )
                atlas[vrc_atlas_index( lay, x, y, z )] =
                    xform_voxel< T >( xform, src[( (size_t)z * atlasDim[1] + y ) * atlasDim[0] + x] );
}
} // namespace

/* the upload transform of `voxelType` on n voxels (dst: the atlas's element, same size as the voxel) */
extern "C" int typed_harness_xform( const void* src, void* dst, uint64_t n, int voxelType )
{
    uint32_t bytes;
    int xform;
    float shift;
    if( !type_traits_of( voxelType, bytes, xform, shift ) )
        return 1;
    for( uint64_t i = 0; i < n; ++i )
    {
        if( bytes == 1 )
            static_cast< uint8_t* >( dst )[i] = xform_voxel< uint8_t >( xform, static_cast< const uint8_t* >( src )[i] );
        else if( bytes == 2 )
            static_cast< uint16_t* >( dst )[i] = xform_voxel< uint16_t >( xform, static_cast< const uint16_t* >( src )[i] );
        else
            static_cast< uint32_t* >( dst )[i] = xform_voxel< uint32_t >( xform, static_cast< const uint32_t* >( src )[i] );
    }
    return 0;
}

/* vrc_classify of n densities: out = n x (r, g, b, a) premultiplied */
extern "C" int typed_harness_classify( const float* tf, const float* d, uint32_t n, float rangeMin, float rangeMax,
                                       float alphaCorrection, int fracBits, float* out )
{
    vrc_lut_params lp;
    lp.rangeMin = rangeMin;
    lp.rangeMax = rangeMax;
    lp.alphaCorrection = alphaCorrection;
    lp.fracBits = fracBits;
    const vrc_classifier cls = vrc_make_classifier( lp );
    vrc_f4 tfp[VRC_TFP_ENTRIES];
    vrc_f2 tfp2[VRC_TFP_ENTRIES];
    for( uint32_t k = 0; k < VRC_TFP_ENTRIES; ++k )
    {
        const uint32_t i = k == 0 ? 0u : ( k - 1u > 255u ? 255u : k - 1u );
        tfp[k] = vrc_f4{ tf[i * 4], tf[i * 4 + 1], tf[i * 4 + 2], tf[i * 4 + 3] };
        tfp2[k] = vrc_f2{ tf[i * 4], tf[i * 4 + 3] };
    }
    for( uint32_t i = 0; i < n; ++i )
    {
        const vrc_f4 e = vrc_classify( tfp, d[i], cls );
        const vrc_f2 g = vrc_classify( tfp2, d[i], cls );
        if( std::memcmp( &g.x, &e.x, 4 ) != 0 || std::memcmp( &g.w, &e.w, 4 ) != 0 )
            return 2; /* the grey form classifies the same bits */
        out[i * 4] = e.x;
        out[i * 4 + 1] = e.y;
        out[i * 4 + 2] = e.z;
        out[i * 4 + 3] = e.w;
    }
    return 0;
}

/* form: bit 0 = grid walk (else reference order), bit 1 = fixed-point stepping, bit 2 = (grey, alpha) form of the point
 * sampler (needs bit 1 and a cleared frame), bit 3 = trilinear filter.  The 1-byte types are classified per sample
 * here too (VRC_MODE_POINT; their table form is tests/cpu_harness/harness.cpp's business). */
extern "C" int typed_harness_render( const void* atlasRowMajor, int voxelType, const uint32_t atlasDim[3],
                                     const uint32_t slotDim[3], float* pixelBuffer, uint32_t W, uint32_t H,
                                     const float* planes, uint32_t nPlanes, const float* tf, const vrc_view_data* view,
                                     uint32_t nNodes, const vrc_node_data* nodes, const vrc_render_data* render, int form,
                                     int fracBits, int clearFirst, uint64_t* samplesOut )
{
    uint32_t bytes;
    int xform;
    float shift;
    if( !type_traits_of( voxelType, bytes, xform, shift ) )
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
    std::vector< uint32_t > atlas32; /* the bits of the float atlas */
    if( bytes == 1 )
        upload< uint8_t >( atlasRowMajor, atlasDim, lay, xform, atlas8 );
    else if( bytes == 2 )
        upload< uint16_t >( atlasRowMajor, atlasDim, lay, xform, atlas16 );
    else
        upload< uint32_t >( atlasRowMajor, atlasDim, lay, xform, atlas32 );
    const float* const atlasF = reinterpret_cast< const float* >( atlas32.data() );

    /* vrc_render: the range moves with the offset-binary voxels */
    vrc_lut_params lp;
    lp.rangeMin = render->dataSourceRange[0] + shift;
    lp.rangeMax = render->dataSourceRange[1] + shift;
    lp.alphaCorrection = (float)render->maxSamplesPerRay / (float)render->samplesPerRay;
    lp.fracBits = fracBits;
    const vrc_classifier cls = vrc_make_classifier( lp );
    std::vector< vrc_f4 > tfp( VRC_TFP_ENTRIES );
    std::vector< vrc_f2 > tfp2( VRC_TFP_ENTRIES );
    const bool grid = ( form & 1 ) != 0, grey = ( form & 4 ) != 0, linear = ( form & 8 ) != 0;
    for( uint32_t k = 0; k < VRC_TFP_ENTRIES; ++k )
    {
        const uint32_t i = k == 0 ? 0u : ( k - 1u > 255u ? 255u : k - 1u );
        tfp[k] = vrc_f4{ tf[i * 4], tf[i * 4 + 1], tf[i * 4 + 2], tf[i * 4 + 3] };
        if( grey && ( tf[i * 4] != tf[i * 4 + 1] || tf[i * 4] != tf[i * 4 + 2] ) )
            return 6;
        tfp2[k] = vrc_f2{ tf[i * 4], tf[i * 4 + 3] };
    }

    vrc_host_tables t;
    vrc_build_tables( geom, nodes, nNodes, t );
    if( grid && !t.gridOk )
        return 2;
    const bool fixed = ( form & 2 ) != 0 && !t.clamp && slotDim[0] <= 248u && slotDim[1] <= 248u && slotDim[2] <= 248u;
    if( grey && ( !fixed || linear || !clearFirst ) )
        return 8;
    float pl[6][4];
    std::memset( pl, 0, sizeof( pl ) );
    for( uint32_t i = 0; i < nPlanes && i < 6; ++i )
        for( int k = 0; k < 4; ++k )
            pl[i][k] = planes[i * 4 + k];
    vrc_frame f;
    std::memset( &f, 0, sizeof( f ) );
    vrc_fill_frame( f, *view, *render, geom, t.g, pl, nPlanes, nNodes, W, H, 0.f, 0.f );
    f.variant = VRC_VARIANT_CUDA;
    f.clearFirst = clearFirst ? 1u : 0u;

    const vrc_f4* const table = grey ? reinterpret_cast< const vrc_f4* >( tfp2.data() ) : tfp.data();
    uint64_t total = 0;
    vrc_f4* pb = reinterpret_cast< vrc_f4* >( pixelBuffer );
    for( uint32_t py = 0; py < H; ++py )
        for( uint32_t px = 0; px < W; ++px )
        {
            uint32_t n = 0;
#define ARGS_DDA( A ) f, t.nodes.data(), t.grid.data(), A, table, cls, pb, px, py, n
#define ARGS_REF( A ) f, t.nodes.data(), A, table, cls, pb, px, py, n
#define FORMS( MODE, FIXED, T, A )                                                                          \
    {                                                                                                       \
        if( grid && t.clamp ) vrc_pixel_grid_dda< true, true, false, MODE, T >( ARGS_DDA( A ) );            \
        else if( grid ) vrc_pixel_grid_dda< false, true, FIXED, MODE, T >( ARGS_DDA( A ) );                 \
        else if( t.clamp ) vrc_pixel_reference_order< true, true, false, MODE, T >( ARGS_REF( A ) );        \
        else vrc_pixel_reference_order< false, true, FIXED, MODE, T >( ARGS_REF( A ) );                     \
    }
#define TYPED( T, A )                                                   \
    {                                                                   \
        if( linear ) FORMS( VRC_MODE_TRILINEAR, false, T, A )           \
        else if( grey ) FORMS( VRC_MODE_POINT_GREY, true, T, A )        \
        else if( fixed ) FORMS( VRC_MODE_POINT, true, T, A )            \
        else FORMS( VRC_MODE_POINT, false, T, A )                       \
    }
            if( bytes == 4 ) TYPED( float, atlasF )
            else if( bytes == 2 ) TYPED( uint16_t, atlas16.data() )
            else TYPED( uint8_t, atlas8.data() )
#undef TYPED
#undef FORMS
#undef ARGS_DDA
#undef ARGS_REF
            total += n;
        }
    if( samplesOut )
        *samplesOut = total;
    return 0;
}
