/*
 * slice_harness.cpp -- host build (g++) of the per-pixel code of a slice frame (libre_amd/csrc/vrc_core.h:
 * vrc_pixel_slice), for tests/test_slice_cpu.py.  TEST INFRASTRUCTURE ONLY: iso_harness.cpp next to it with the slice's
 * plane in place of the isovalue and no gradient.
 *
 * A row-major atlas of uint8, uint16 or float voxels goes into the micro-blocked layout; the uniformity word the brick
 * upload leaves per slot on the GPU is reduced here over each slot's brick, and the frame is rendered by the instance
 * the launcher of vrc_kernels_slice.hip picks.
 *
 * With -DSLICE_HARNESS_MAIN the file is a program of its own: a small volume through every sampler, for a run under
 * -fsanitize=address,undefined.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vrc_hip.h"
#include "../../libre_amd/csrc/vrc_tables.h"

namespace
{
template < typename T >
void upload( const void* rowMajor, const uint32_t atlasDim[3], const vrc_layout& lay, const uint32_t brick[3],
             std::vector< T >& atlas, std::vector< uint32_t >& info )
{
    const T* const src = static_cast< const T* >( rowMajor );
    atlas.resize( (size_t)atlasDim[0] * atlasDim[1] * atlasDim[2] );
    const uint32_t nSlots = lay.slots[0] * lay.slots[1] * lay.slots[2];
    info.assign( nSlots, 0u );
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
                    continue; /* slot padding */
                const uint32_t slot = ( k * lay.slots[1] + j ) * lay.slots[0] + i;
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

/* mipMax, mipDepth: W x H running V bits and D of the passes (first != 0: not read).  plane: vrc_set_slice's (the scenes
 * here hold unsigned voxels: no shift).  form: bit 0 = grid form (else reference order, every node a candidate: the tile
 * culling is the kernel's), bit 3 = trilinear samples, bit 5 = uniform bricks.  voxelBytes: 1, 2 or 4 (float).  values,
 * counts: W x H entries, what vrc_get_projection_values returns after this pass. */
extern "C" int slice_harness_render( const void* atlasRowMajor, uint32_t voxelBytes, const uint32_t atlasDim[3],
                                    const uint32_t slotDim[3], const uint32_t brickDim[3], float* pixelBuffer,
                                    uint32_t* mipMax, float* mipDepth, const float plane[4], uint32_t W, uint32_t H,
                                    const float* planes, uint32_t nPlanes, const float* tf, const vrc_view_data* view,
                                    uint32_t nNodes, const vrc_node_data* nodes, const vrc_render_data* render, int form,
                                    int fracBits, int first, uint64_t* samplesOut, float* values, uint32_t* counts )
{
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
    std::vector< uint32_t > atlas32, info;
    if( voxelBytes == 1 )
        upload< uint8_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas8, info );
    else if( voxelBytes == 2 )
        upload< uint16_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas16, info );
    else if( voxelBytes == 4 )
        upload< uint32_t >( atlasRowMajor, atlasDim, lay, brickDim, atlas32, info );
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
    f.mipDepth = mipDepth;
    for( int k = 0; k < 4; ++k )
        f.slicePlane[k] = plane[k];
    f.slotInfo = ( form & 32 ) ? info.data() : nullptr;

    uint64_t total = 0;
    vrc_f4* pb = reinterpret_cast< vrc_f4* >( pixelBuffer );
    for( uint32_t py = 0; py < H; ++py )
        for( uint32_t px = 0; px < W; ++px )
        {
            uint32_t n = 0;
#define ARGS( A ) f, t.nodes.data(), t.grid.data(), A, tfp.data(), cls, pb, px, py, n
#define TYPED( T, A )                                                          \
    {                                                                          \
        if( grid && linear ) vrc_pixel_slice< true, true, T, false >( ARGS( A ) );   \
        else if( grid ) vrc_pixel_slice< true, false, T, false >( ARGS( A ) );       \
        else if( linear ) vrc_pixel_slice< false, true, T, false >( ARGS( A ) );     \
        else vrc_pixel_slice< false, false, T, false >( ARGS( A ) );                 \
    }
            if( voxelBytes == 4 ) TYPED( float, atlasF )
            else if( voxelBytes == 2 ) TYPED( uint16_t, atlas16.data() )
            else TYPED( uint8_t, atlas8.data() )
#undef TYPED
#undef ARGS
            total += n;
            const size_t i = (size_t)py * W + px;
            if( values && counts )
                vrc_projection_value( (uint32_t)VRC_FOLD_FIRST, linear || voxelBytes == 4, 0.0f, mipMax[i], 0ull, 0u, values[i], counts[i] );
        }
    if( samplesOut )
        *samplesOut = total;
    return 0;
}

#ifdef SLICE_HARNESS_MAIN
/* One brick of 16^3 in a slot of 16^3 (no overlap: every sample near a face clamps), planes through its middle, its faces
 * and beyond them, every voxel type, both filters and both forms, first and later passes */
int main()
{
    const uint32_t dim[3] = { 16u, 16u, 16u };
    std::vector< float > volF( 16 * 16 * 16 );
    std::vector< uint16_t > vol16( volF.size() );
    std::vector< uint8_t > vol8( volF.size() );
    for( size_t i = 0; i < volF.size(); ++i )
    {
        vol8[i] = (uint8_t)( i * 7u );
        vol16[i] = (uint16_t)( i * 257u );
        volF[i] = (float)i * 0.25f - 100.0f;
    }
    volF[5] = NAN;
    const uint32_t W = 19, H = 13;
    vrc_view_data view;
    std::memset( &view, 0, sizeof( view ) );
    view.eyePosition[2] = 1.5f;
    view.glViewport[2] = W;
    view.glViewport[3] = H;
    /* a frustum of +-0.05 at near 0.1 looking down -z from (0, 0, 1.5): inverse projection and inverse view */
    const float n = 0.1f, fa = 15.0f, r = 0.05f;
    const float proj[16] = { n / r, 0, 0, 0, 0, n / r, 0, 0, 0, 0, -( fa + n ) / ( fa - n ), -1.0f, 0, 0, -2.0f * fa * n / ( fa - n ), 0 };
    /* inverse of that perspective matrix (column-major) */
    float inv[16];
    std::memset( inv, 0, sizeof( inv ) );
    inv[0] = 1.0f / proj[0];
    inv[5] = 1.0f / proj[5];
    inv[11] = 1.0f / proj[14];
    inv[14] = -1.0f;
    inv[15] = proj[10] / proj[14];
    std::memcpy( view.invProjMatrix, inv, sizeof( inv ) );
    float iv[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1.5f, 1 };
    std::memcpy( view.invViewMatrix, iv, sizeof( iv ) );
    for( int a = 0; a < 3; ++a )
    {
        view.aabbMin[a] = -0.5f;
        view.aabbMax[a] = 0.5f;
    }
    view.nearPlane = n;
    vrc_node_data node;
    std::memset( &node, 0, sizeof( node ) );
    for( int a = 0; a < 3; ++a )
    {
        node.aabbMin[a] = -0.5f;
        node.aabbSize[a] = 1.0f;
        node.textureMin[a] = 0.0f;
        node.textureSize[a] = 1.0f;
    }
    vrc_render_data render;
    std::memset( &render, 0, sizeof( render ) );
    render.samplesPerRay = 32;
    render.maxSamplesPerRay = 32;
    render.samplesPerPixel = 1;
    render.dataSourceRange[0] = 0.0f;
    render.dataSourceRange[1] = 255.0f;
    std::vector< float > tf( 256 * 4 );
    for( int i = 0; i < 256; ++i )
        tf[4 * i] = tf[4 * i + 1] = tf[4 * i + 2] = tf[4 * i + 3] = (float)i / 255.0f;
    const float planesZ[][4] = { { 0, 0, 1, 0 }, { 0, 0, 1, 0.5f }, { 0, 0, 1, -0.5f }, { 0.3f, -0.2f, 1, 0.1f }, { 1, 0, 0, 0 }, { 0, 0, 1, 3.0f } };
    uint64_t sampled = 0;
    for( uint32_t bytes = 1; bytes <= 4; bytes *= 2 )
        for( int form = 0; form < 64; ++form )
        {
            if( form & ( 2 | 4 | 16 ) )
                continue;
            for( const auto& p : planesZ )
            {
                std::vector< float > fb( W * H * 4, 0.0f ), dep( W * H ), values( W * H );
                std::vector< uint32_t > run( W * H ), counts( W * H );
                const void* vol = bytes == 1 ? (const void*)vol8.data() : bytes == 2 ? (const void*)vol16.data() : (const void*)volF.data();
                for( int first = 1; first >= 0; --first )
                {
                    uint64_t s = 0;
                    const int rc = slice_harness_render( vol, bytes, dim, dim, dim, fb.data(), run.data(), dep.data(), p, W, H, nullptr, 0,
                                                         tf.data(), &view, 1, &node, &render, form, 8, first, &s, values.data(),
                                                         counts.data() );
                    if( rc != 0 )
                    {
                        std::printf( "slice_harness_render: %d\n", rc );
                        return 1;
                    }
                    if( !first && s != 0 )
                    {
                        std::printf( "a second pass over the same node sampled %llu pixels again\n", (unsigned long long)s );
                        return 1;
                    }
                    sampled += s;
                }
            }
        }
    std::printf( "slice harness: %llu pixels sampled\n", (unsigned long long)sampled );
    return sampled != 0 ? 0 : 1;
}
#endif
