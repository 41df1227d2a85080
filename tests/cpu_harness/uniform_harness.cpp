/*
 * uniform_harness.cpp -- host build (g++) of the per-ray code of libre_amd/csrc/vrc_core.h with the per-slot
 * uniformity words (vrc_frame::slotInfo, vrc_dev_node::slotInfoIndex) that the brick upload writes on the GPU, for
 * tests/test_uniform_bricks_cpu.py.  TEST INFRASTRUCTURE ONLY, like harness.cpp next to it.
 *
 * The words are derived here the way vrc_k_repack_u8x8 derives them: a slot whose voxels all equal its first voxel is
 * KNOWN with that value, any other slot KNOWN | MIXED.  With `poison` the voxels of every uniform slot are then
 * overwritten with another value: a frame that still equals the general march's proves that the uniform march does
 * not read the atlas.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../libre_amd/csrc/vrc_tables.h"

/* form: bit 0 = grid walk (else reference order), bit 1 = fixed-point stepping, bit 2 = (grey, alpha) table form,
 * bit 3 = per-ray LOD (then bit 0 is ignored).  useInfo: 0 = no words (the general march for every brick), 1 = words,
 * 2 = words + poisoned uniform slots.  uniformSlotsOut: how many slots hold one value. */
extern "C" int uniform_harness_render( const uint8_t* atlasRowMajor, const uint32_t atlasDim[3], const uint32_t slotDim[3],
                                       float* pixelBuffer, uint32_t W, uint32_t H, const float* planes, uint32_t nPlanes,
                                       const float* tf, const vrc_view_data* view, uint32_t nNodes,
                                       const vrc_node_data* nodes, const vrc_render_data* render, int form, int useInfo,
                                       int clearFirst, float lodSse, float lodWorldPerPixel, uint64_t* samplesOut,
                                       uint32_t* uniformSlotsOut )
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
    const size_t nVoxels = (size_t)atlasDim[0] * atlasDim[1] * atlasDim[2];
    std::vector< uint8_t > atlas( nVoxels );
    for( uint32_t z = 0; z < atlasDim[2]; ++z )
        for( uint32_t y = 0; y < atlasDim[1]; ++y )
            for( uint32_t x = 0; x < atlasDim[0]; ++x )
                atlas[vrc_atlas_index( lay, x, y, z )] = atlasRowMajor[( (size_t)z * atlasDim[1] + y ) * atlasDim[0] + x];

    /* the uniformity words, slot ordinal x fastest (vrc_build_tables) */
    const size_t slotElems = (size_t)slotDim[0] * slotDim[1] * slotDim[2];
    std::vector< uint32_t > info( (size_t)geom.slots[0] * geom.slots[1] * geom.slots[2] );
    uint32_t nUniform = 0;
    for( uint32_t k = 0; k < geom.slots[2]; ++k )
        for( uint32_t j = 0; j < geom.slots[1]; ++j )
            for( uint32_t i = 0; i < geom.slots[0]; ++i )
            {
                uint8_t* const v = atlas.data() + vrc_slot_base( lay, i, j, k );
                bool mixed = false;
                for( size_t e = 1; e < slotElems; ++e )
                    mixed = mixed || v[e] != v[0];
                info[( (size_t)k * geom.slots[1] + j ) * geom.slots[0] + i] =
                    (uint32_t)v[0] | VRC_SLOT_KNOWN | ( mixed ? VRC_SLOT_MIXED : 0u );
                if( !mixed )
                {
                    ++nUniform;
                    if( useInfo == 2 )
                        std::memset( v, v[0] ^ 0x5A, slotElems );
                }
            }
    if( uniformSlotsOut )
        *uniformSlotsOut = nUniform;

    vrc_lut_params lp;
    lp.rangeMin = render->dataSourceRange[0];
    lp.rangeMax = render->dataSourceRange[1];
    lp.alphaCorrection = (float)render->maxSamplesPerRay / (float)render->samplesPerRay;
    lp.fracBits = 8;
    const bool rayLod = ( form & 8 ) != 0, grey = ( form & 4 ) != 0, fixedAsked = ( form & 2 ) != 0;
    const uint32_t lutLevels = rayLod ? (uint32_t)VRC_MAX_LOD_LEVELS : 1u;
    std::vector< vrc_f4 > lut( lutLevels * VRC_LUT_ENTRIES );
    for( uint32_t j = 0; j < lutLevels; ++j )
    {
        vrc_lut_params lj = lp;
        lj.alphaCorrection = lp.alphaCorrection * (float)( 1u << j );
        for( uint32_t d = 0; d < 256; ++d )
            lut[j * VRC_LUT_ENTRIES + d] = vrc_lut_entry( tf, d, lj );
        lut[j * VRC_LUT_ENTRIES + 256] = vrc_f4{ 0.f, 0.f, 0.f, 0.f };
    }
    /* the (grey, alpha) form of the same tables, as the kernels stage it */
    std::vector< vrc_f2 > lut2( lut.size() );
    for( size_t i = 0; i < lut.size(); ++i )
    {
        if( grey && ( lut[i].x != lut[i].y || lut[i].x != lut[i].z ) )
            return 6;
        lut2[i] = vrc_f2{ lut[i].x, lut[i].w };
    }

    vrc_host_tables t;
    vrc_build_tables( geom, nodes, nNodes, t );
    if( rayLod )
        vrc_build_lod_tables( geom, nodes, nNodes, t );
    if( t.clamp || ( rayLod ? !t.lodOk : ( ( form & 1 ) && !t.gridOk ) ) )
        return 2;
    for( const vrc_dev_node& n : t.nodes )
        if( n.slotInfoIndex == 0u || n.slotInfoIndex > info.size() )
            return 7;
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
    f.slotInfo = useInfo ? info.data() : nullptr;
    if( rayLod )
    {
        f.lodLevels = t.lodLevels;
        f.lodBase = (float)( t.finestVoxelWorld / ( (double)lodSse * (double)lodWorldPerPixel ) );
    }
    if( grey && !clearFirst )
        return 8; /* the grey form starts from a cleared (grey) pixel */

    const vrc_classifier cls = vrc_make_classifier( lp );
    const vrc_f4* const table = grey ? reinterpret_cast< const vrc_f4* >( lut2.data() ) : lut.data();
    uint64_t total = 0;
    vrc_f4* pb = reinterpret_cast< vrc_f4* >( pixelBuffer );
    for( uint32_t py = 0; py < H; ++py )
        for( uint32_t px = 0; px < W; ++px )
        {
            uint32_t n = 0;
#define ARGS_DDA f, t.nodes.data(), t.grid.data(), atlas.data(), table, cls, pb, px, py, n
#define ARGS_REF f, t.nodes.data(), atlas.data(), table, cls, pb, px, py, n
#define FORMS( MODE )                                                                                              \
    {                                                                                                              \
        if( rayLod && fixedAsked ) vrc_pixel_ray_lod< false, true, true, MODE, uint8_t >( ARGS_DDA );              \
        else if( rayLod ) vrc_pixel_ray_lod< false, true, false, MODE, uint8_t >( ARGS_DDA );                      \
        else if( ( form & 1 ) && fixedAsked ) vrc_pixel_grid_dda< false, true, true, MODE, uint8_t >( ARGS_DDA );  \
        else if( form & 1 ) vrc_pixel_grid_dda< false, true, false, MODE, uint8_t >( ARGS_DDA );                   \
        else if( fixedAsked ) vrc_pixel_reference_order< false, true, true, MODE, uint8_t >( ARGS_REF );           \
        else vrc_pixel_reference_order< false, true, false, MODE, uint8_t >( ARGS_REF );                           \
    }
            if( grey ) FORMS( VRC_MODE_GREY )
            else FORMS( VRC_MODE_TABLE )
#undef FORMS
#undef ARGS_DDA
#undef ARGS_REF
            total += n;
        }
    if( samplesOut )
        *samplesOut = total;
    return 0;
}
