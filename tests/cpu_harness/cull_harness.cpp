/*
 * cull_harness.cpp -- host build (g++, and clang -mfma) of the tile culling of the reference-order kernels
 * (libre_amd/csrc/vrc_core.h, "tile culling": vrc_make_tile_pyramid, vrc_pyramid_may_hit), for
 * tests/test_tile_cull_cpu.py and tests/test_tile_cull.py.  TEST INFRASTRUCTURE ONLY.
 *
 * The five kernels that carry the block (vrc_k_raycast and _preint their own copies in libre_amd/csrc/vrc_kernels.hip and
 * vrc_kernels_preint.hip; _mip, _shade and _cdepth the shared one, libre_amd/csrc/vrc_kernel_frame.h:
 * vrc_frame_cull_tile) run it per wave: the wave's
 * 8x8 tile, a pyramid through its corner pixels with one pixel of margin, the list tested 64 bricks at a time, the
 * survivors compacted by ballot into 16-bit indices.  cull_tile() below restates that loop in plain C++ -- lanes
 * become an inner loop, the ballot a running count -- and calls the product's own pyramid functions.  The rule that
 * picks one of the four regimes is restated with it; tests/test_tile_cull_cpu.py reads the kernel sources to check
 * that the constants here are the ones all three copies carry, and that every other kernel calls the shared one.
 *
 * tests/host_san/cull_selftest.cpp includes this file and adds a main(): the stand-alone program for the address and
 * undefined-behaviour sanitizers.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/vrc_hip.h"
#include "../../libre_amd/csrc/vrc_tables.h"

/* the wave's tile (vrc_internal.h: VRC_TILE_W x VRC_TILE_H) and the bounds of the culled regime as the kernels have
 * them: `f.nodeCount > 8u && f.nodeCount <= 65535u` */
#define CULL_TILE_W 8u
#define CULL_TILE_H 8u
#define CULL_LOWER 8u
#define CULL_UPPER 65535u

enum
{
    CULL_REGIME_SHORT = 0,   /* nodeCount <= CULL_LOWER: the plain loop */
    CULL_REGIME_CULLED = 1,  /* the loop over the tile's candidates */
    CULL_REGIME_OVERFLOW = 2, /* more than VRC_TILE_CANDIDATES survivors: the plain loop */
    CULL_REGIME_LONG = 3     /* more than CULL_UPPER entries: the plain loop */
};

namespace
{
struct cull_setup
{
    vrc_atlas_geom geom;
    vrc_layout lay;
    vrc_host_tables t;
    vrc_frame f;
};

/* tables and frame as harness.cpp makes them; rowMap: the frame row of every local row (H entries), or null */
int prepare( cull_setup& c, const uint32_t atlasDim[3], const uint32_t slotDim[3], uint32_t W, uint32_t H, const float* planes,
             uint32_t nPlanes, const vrc_view_data* view, uint32_t nNodes, const vrc_node_data* nodes,
             const vrc_render_data* render, const uint32_t* rowMap, int variant, int pixelOffX, int pixelOffY )
{
    for( int a = 0; a < 3; ++a )
    {
        if( atlasDim[a] % 8u || slotDim[a] % 8u || atlasDim[a] % slotDim[a] )
            return 1;
        c.geom.atlasDim[a] = atlasDim[a];
        c.geom.slotDim[a] = c.lay.slotDim[a] = slotDim[a];
        c.geom.slots[a] = c.lay.slots[a] = atlasDim[a] / slotDim[a];
    }
    vrc_build_tables( c.geom, nodes, nNodes, c.t );
    float pl[6][4];
    std::memset( pl, 0, sizeof( pl ) );
    for( uint32_t i = 0; i < nPlanes && i < 6; ++i )
        for( int k = 0; k < 4; ++k )
            pl[i][k] = planes[i * 4 + k];
    std::memset( &c.f, 0, sizeof( c.f ) );
    const float centre = variant == 1 ? 0.5f : 0.0f; /* glRaycaster: gl_FragCoord */
    vrc_fill_frame( c.f, *view, *render, c.geom, c.t.g, pl, nPlanes, nNodes, W, H, (float)pixelOffX + centre,
                    (float)pixelOffY + centre );
    c.f.variant = variant == 1 ? VRC_VARIANT_GL : VRC_VARIANT_CUDA;
    c.f.samplesPerPixel = ( variant == 1 && render->samplesPerPixel > 1u ) ? render->samplesPerPixel : 1u;
    c.f.rowMap = rowMap;
    return 0;
}

/* The wave's block, statement for statement (vrc_kernel_frame.h: vrc_frame_cull_tile): the pyramid of tile (tx, ty),
 * the list against it in steps of 64, the survivors into mine[0 .. VRC_TILE_CANDIDATES).  kept (nodeCount bytes, or
 * null): 1 where the pyramid keeps the brick.  Returns the survivor count.  The test itself does not depend on the
 * regime; which loop the lanes then run is cull_regime(). */
uint32_t cull_tile( const vrc_frame& f, const vrc_dev_node* nodes, uint32_t tx, uint32_t ty, uint16_t* mine, uint8_t* kept )
{
    /* frame rows of the tile (row bands: local rows map to frame rows, not always consecutive ones) */
    float r0 = 1e30f, r1 = -1e30f;
    for( uint32_t j = 0; j < CULL_TILE_H; ++j )
    {
        const uint32_t ly = ty * CULL_TILE_H + j;
        if( ly < f.height )
        {
            const float fr = (float)( f.rowMap ? f.rowMap[ly] : ly );
            r0 = fminf( r0, fr );
            r1 = fmaxf( r1, fr );
        }
    }
    const vrc_tile_pyramid pyr = vrc_make_tile_pyramid( f, (float)( tx * CULL_TILE_W ) - 1.0f, r0 - 1.0f,
                                                       (float)( tx * CULL_TILE_W + CULL_TILE_W ), r1 + 1.0f );
    uint32_t nCand = 0;
    for( uint32_t base = 0; base < f.nodeCount; base += 64u )
    {
        uint32_t before = 0; /* the lanes below this one that keep their brick (mbcnt of the ballot) */
        for( uint32_t lane = 0; lane < 64u; ++lane )
        {
            const uint32_t i = base + lane;
            bool in = false;
            if( i < f.nodeCount )
                in = vrc_pyramid_may_hit( pyr, nodes[i].aabbMin, nodes[i].aabbSize );
            const uint32_t at = nCand + before;
            if( in && at < VRC_TILE_CANDIDATES && mine )
                mine[at] = (uint16_t)i;
            if( in && kept )
                kept[i] = 1;
            before += in ? 1u : 0u;
        }
        nCand += before;
    }
    return nCand;
}

int cull_regime( uint32_t nodeCount, uint32_t nCand )
{
    if( !( nodeCount > CULL_LOWER ) )
        return CULL_REGIME_SHORT;
    if( !( nodeCount <= CULL_UPPER ) )
        return CULL_REGIME_LONG;
    return nCand <= VRC_TILE_CANDIDATES ? CULL_REGIME_CULLED : CULL_REGIME_OVERFLOW;
}

/* hit | stop of one ray against one brick: bit 0 = vrc_brick_segment returns true, bit 1 = it sets `stop` */
uint8_t ray_needs( const vrc_frame& f, const vrc_ray& r, const vrc_dev_node& n )
{
    vrc_segment s;
    bool stop = false;
    const bool hit = vrc_brick_segment( f, r, n, f.stepSize, &s, &stop );
    return (uint8_t)( ( hit ? 1u : 0u ) | ( stop ? 2u : 0u ) );
}

template < typename T >
void micro_block( const void* rowMajor, const uint32_t atlasDim[3], const vrc_layout& lay, std::vector< T >& atlas )
{
    const T* const src = static_cast< const T* >( rowMajor );
    atlas.resize( (size_t)atlasDim[0] * atlasDim[1] * atlasDim[2] );
    for( uint32_t z = 0; z < atlasDim[2]; ++z )
        for( uint32_t y = 0; y < atlasDim[1]; ++y )
            for( uint32_t x = 0; x < atlasDim[0]; ++x )
                atlas[vrc_atlas_index( lay, x, y, z )] = src[( (size_t)z * atlasDim[1] + y ) * atlasDim[0] + x];
}

/* one pixel through the instance the launchers pick: mode 0 the classified table (8-bit voxels), 1 point samples
 * classified one by one, 2 trilinear gathers, 3 / 4 the shaded composite with point / trilinear samples */
template < typename T >
int pixel( const vrc_frame& f, const vrc_host_tables& t, const T* atlas, const vrc_f4* table, const vrc_classifier& cls, vrc_f4* pb,
           uint32_t px, uint32_t py, uint32_t& n, int mode, const uint16_t* cand, uint32_t nCand )
{
#define FORM( MODE )                                                                                                              \
    {                                                                                                                             \
        if( t.clamp ) vrc_pixel_reference_order< true, true, false, MODE, T >( f, t.nodes.data(), atlas, table, cls, pb, px, py, n, cand, nCand ); \
        else vrc_pixel_reference_order< false, true, false, MODE, T >( f, t.nodes.data(), atlas, table, cls, pb, px, py, n, cand, nCand );       \
        return 0;                                                                                                                 \
    }
    if constexpr( sizeof( T ) == 1 )
        if( mode == 0 ) FORM( VRC_MODE_TABLE )
    if( mode == 1 ) FORM( VRC_MODE_POINT )
    if( mode == 2 ) FORM( VRC_MODE_TRILINEAR )
    if( mode == 3 ) FORM( VRC_MODE_SHADE )
    if( mode == 4 ) FORM( VRC_MODE_SHADE_TRILINEAR )
#undef FORM
    return 1;
}
} // namespace

/* out[0 .. 5): VRC_TILE_CANDIDATES, the lower and the upper bound of the culled regime, the tile's width and height */
extern "C" void cull_limits( uint32_t out[5] )
{
    out[0] = VRC_TILE_CANDIDATES;
    out[1] = CULL_LOWER;
    out[2] = CULL_UPPER;
    out[3] = CULL_TILE_W;
    out[4] = CULL_TILE_H;
}

/* The product's test by itself: the pyramid through the window positions (x0, y0) .. (x1, y1) of this view, against n
 * boxes (min[3], size[3] each); out[i] = 1 where vrc_pyramid_may_hit keeps box i. */
extern "C" int cull_pyramid_keeps( uint32_t W, uint32_t H, const vrc_view_data* view, const vrc_render_data* render, int variant,
                                  float x0, float y0, float x1, float y1, const float* boxes, uint32_t n, uint8_t* out )
{
    const uint32_t dim[3] = { 8u, 8u, 8u };
    cull_setup c;
    if( const int rc = prepare( c, dim, dim, W, H, nullptr, 0, view, 0, nullptr, render, nullptr, variant, 0, 0 ) )
        return rc;
    const vrc_tile_pyramid pyr = vrc_make_tile_pyramid( c.f, x0, y0, x1, y1 );
    for( uint32_t i = 0; i < n; ++i )
        out[i] = vrc_pyramid_may_hit( pyr, boxes + 6u * i, boxes + 6u * i + 3u ) ? 1 : 0;
    return 0;
}

/* tiles: nTiles tile indices (ty * tilesX + tx), or null for every tile of the W x H buffer in that order.
 * kept: nTiles x nNodes bytes (1 = the pyramid keeps the brick), counts: nTiles survivor counts, regimes: nTiles of
 * CULL_REGIME_*; each may be null. */
extern "C" int cull_tile_masks( const uint32_t atlasDim[3], const uint32_t slotDim[3], uint32_t W, uint32_t H, const float* planes,
                               uint32_t nPlanes, const vrc_view_data* view, uint32_t nNodes, const vrc_node_data* nodes,
                               const vrc_render_data* render, const uint32_t* rowMap, int variant, int pixelOffX,
                               int pixelOffY, const uint32_t* tiles, uint32_t nTiles, uint8_t* kept, uint32_t* counts,
                               int32_t* regimes )
{
    cull_setup c;
    if( const int rc = prepare( c, atlasDim, slotDim, W, H, planes, nPlanes, view, nNodes, nodes, render, rowMap, variant, pixelOffX, pixelOffY ) )
        return rc;
    const uint32_t tilesX = ( W + CULL_TILE_W - 1u ) / CULL_TILE_W, tilesY = ( H + CULL_TILE_H - 1u ) / CULL_TILE_H;
    if( !tiles )
        nTiles = tilesX * tilesY;
    for( uint32_t k = 0; k < nTiles; ++k )
    {
        const uint32_t tile = tiles ? tiles[k] : k;
        if( tile >= tilesX * tilesY )
            return 2;
        uint8_t* const row = kept ? kept + (size_t)k * nNodes : nullptr;
        if( row )
            std::memset( row, 0, nNodes );
        const uint32_t n = cull_tile( c.f, c.t.nodes.data(), tile % tilesX, tile / tilesX, nullptr, row );
        if( counts )
            counts[k] = n;
        if( regimes )
            regimes[k] = cull_regime( nNodes, n );
    }
    return 0;
}

/* needed: nTiles x nNodes bytes -- bit 0: some in-frame pixel of the tile has a ray that vrc_brick_segment marches
 * through the brick; bit 1: some ray for which it sets `stop` (the reference's loop ends there).  The rays are those
 * of vrc_pixel_reference_order: one per pixel, or under the glRaycaster variant with samplesPerPixel > 1 the jittered
 * rays of vrc_pixel_gl_supersampled.  Rays that miss the volume test no brick. */
extern "C" int cull_needed( const uint32_t atlasDim[3], const uint32_t slotDim[3], uint32_t W, uint32_t H, const float* planes,
                           uint32_t nPlanes, const vrc_view_data* view, uint32_t nNodes, const vrc_node_data* nodes,
                           const vrc_render_data* render, const uint32_t* rowMap, int variant, int pixelOffX, int pixelOffY,
                           const uint32_t* tiles, uint32_t nTiles, uint8_t* needed )
{
    cull_setup c;
    if( const int rc = prepare( c, atlasDim, slotDim, W, H, planes, nPlanes, view, nNodes, nodes, render, rowMap, variant, pixelOffX, pixelOffY ) )
        return rc;
    const vrc_frame& f = c.f;
    const uint32_t tilesX = ( W + CULL_TILE_W - 1u ) / CULL_TILE_W, tilesY = ( H + CULL_TILE_H - 1u ) / CULL_TILE_H;
    if( !tiles )
        nTiles = tilesX * tilesY;
    std::vector< vrc_ray > rays;
    for( uint32_t k = 0; k < nTiles; ++k )
    {
        const uint32_t tile = tiles ? tiles[k] : k;
        if( tile >= tilesX * tilesY )
            return 2;
        const uint32_t tx = tile % tilesX, ty = tile / tilesX;
        rays.clear();
        for( uint32_t ly = 0; ly < CULL_TILE_H; ++ly )
            for( uint32_t lx = 0; lx < CULL_TILE_W; ++lx )
            {
                const uint32_t px = tx * CULL_TILE_W + lx, py = ty * CULL_TILE_H + ly;
                if( !( px < f.width && py < f.height ) )
                    continue;
                const uint32_t row = f.rowMap ? f.rowMap[py] : py;
                if( f.variant == VRC_VARIANT_GL && f.samplesPerPixel > 1u )
                {
                    const float fx = (float)px + f.pixelOffX, fy = (float)row + f.pixelOffY;
                    for( uint32_t j = 0; j < f.samplesPerPixel; ++j )
                    {
                        const float fk = (float)j;
                        const float dx = vrc_gl_rand( fx * fk, fy * fk ) / 2.0f;
                        const float dy = vrc_gl_rand( fx * 2.0f * fk, fy * 2.0f * fk ) / 2.0f;
                        rays.push_back( vrc_setup_ray_at( f, fx + dx, fy + dy ) );
                    }
                }
                else
                    rays.push_back( vrc_setup_ray( f, px, row ) );
            }
        uint8_t* const out = needed + (size_t)k * nNodes;
        for( uint32_t i = 0; i < nNodes; ++i )
        {
            uint8_t bits = 0;
            for( const vrc_ray& r : rays )
                if( r.hit )
                    bits |= ray_needs( f, r, c.t.nodes[i] );
            out[i] = bits;
        }
    }
    return 0;
}

/* The frame of vrc_pixel_reference_order over the W x H buffer, tile by tile as the kernels run it.  culled != 0: every
 * tile takes the loop its regime selects (the candidates in list order where it is the culled one); culled == 0: every
 * tile runs the plain loop (candidates = nullptr).  pixelBuffer is read and written (a frame of several passes
 * accumulates in it).  tiles: as for cull_tile_masks (the pixels of other tiles are left alone).  mode: see pixel().
 * regimes: one CULL_REGIME_* per rendered tile, or null. */
extern "C" int cull_render( const void* atlasRowMajor, uint32_t voxelBytes, const uint32_t atlasDim[3], const uint32_t slotDim[3],
                           float* pixelBuffer, uint32_t W, uint32_t H, const float* planes, uint32_t nPlanes, const float* tf,
                           const vrc_view_data* view, uint32_t nNodes, const vrc_node_data* nodes,
                           const vrc_render_data* render, const uint32_t* rowMap, int variant, int pixelOffX, int pixelOffY,
                           const uint32_t* tiles, uint32_t nTiles, int mode, float ambient, int culled, uint64_t* samplesOut,
                           int32_t* regimes )
{
    if( ( voxelBytes != 1 && voxelBytes != 2 ) || ( voxelBytes == 2 && mode == 0 ) || mode < 0 || mode > 4 )
        return 3;
    if( mode >= 3 && variant != 0 )
        return 3; /* a shaded frame is defined on the cudaRaycaster variant */
    cull_setup c;
    if( const int rc = prepare( c, atlasDim, slotDim, W, H, planes, nPlanes, view, nNodes, nodes, render, rowMap, variant, pixelOffX, pixelOffY ) )
        return rc;
    vrc_frame& f = c.f;
    f.shadeAmbient = mode >= 3 ? ambient : 0.0f;
    std::vector< uint8_t > atlas8;
    std::vector< uint16_t > atlas16;
    if( voxelBytes == 1 )
        micro_block< uint8_t >( atlasRowMajor, atlasDim, c.lay, atlas8 );
    else
        micro_block< uint16_t >( atlasRowMajor, atlasDim, c.lay, atlas16 );

    vrc_lut_params lp;
    lp.rangeMin = render->dataSourceRange[0];
    lp.rangeMax = render->dataSourceRange[1];
    lp.alphaCorrection = (float)render->maxSamplesPerRay / (float)render->samplesPerRay;
    lp.fracBits = 8;
    const vrc_classifier cls = vrc_make_classifier( lp );
    std::vector< vrc_f4 > lut( VRC_TFP_ENTRIES ), tfp( VRC_TFP_ENTRIES );
    for( uint32_t d = 0; d < 256; ++d )
        lut[d] = vrc_lut_entry( tf, d, lp );
    lut[256] = lut[257] = vrc_f4{ 0.f, 0.f, 0.f, 0.f };
    for( uint32_t k = 0; k < VRC_TFP_ENTRIES; ++k )
    {
        const uint32_t i = k == 0 ? 0u : ( k - 1u > 255u ? 255u : k - 1u );
        tfp[k] = vrc_f4{ tf[i * 4], tf[i * 4 + 1], tf[i * 4 + 2], tf[i * 4 + 3] };
    }
    /* the classified table serves 8-bit point samples (modes 0 and 3); every other form classifies per sample */
    const bool classified = voxelBytes == 1 && ( mode == 0 || mode == 3 );
    const vrc_f4* const table = classified ? lut.data() : tfp.data();

    const uint32_t tilesX = ( W + CULL_TILE_W - 1u ) / CULL_TILE_W, tilesY = ( H + CULL_TILE_H - 1u ) / CULL_TILE_H;
    std::vector< uint16_t > mine( VRC_TILE_CANDIDATES ); /* the wave's array: exactly its size */
    vrc_f4* const pb = reinterpret_cast< vrc_f4* >( pixelBuffer );
    uint64_t total = 0;
    if( !tiles )
        nTiles = tilesX * tilesY;
    for( uint32_t k = 0; k < nTiles; ++k )
    {
        const uint32_t tile = tiles ? tiles[k] : k;
        if( tile >= tilesX * tilesY )
            return 2;
        const uint32_t tx = tile % tilesX, ty = tile / tilesX;
        const uint16_t* cand = nullptr;
        uint32_t nCand = 0;
        int regime = cull_regime( nNodes, 0u );
        if( f.nodeCount > CULL_LOWER && f.nodeCount <= CULL_UPPER )
        {
            nCand = cull_tile( f, c.t.nodes.data(), tx, ty, mine.data(), nullptr );
            regime = cull_regime( nNodes, nCand );
            if( nCand <= VRC_TILE_CANDIDATES )
                cand = mine.data();
        }
        if( regimes )
            regimes[k] = regime;
        if( !culled )
            cand = nullptr;
        for( uint32_t ly = 0; ly < CULL_TILE_H; ++ly )
            for( uint32_t lx = 0; lx < CULL_TILE_W; ++lx )
            {
                const uint32_t px = tx * CULL_TILE_W + lx, py = ty * CULL_TILE_H + ly;
                if( !( px < f.width && py < f.height ) )
                    continue;
                uint32_t n = 0;
                const int rc = voxelBytes == 1 ? pixel< uint8_t >( f, c.t, atlas8.data(), table, cls, pb, px, py, n, mode, cand, nCand )
                                               : pixel< uint16_t >( f, c.t, atlas16.data(), table, cls, pb, px, py, n, mode, cand, nCand );
                if( rc )
                    return 3;
                total += n;
            }
    }
    if( samplesOut )
        *samplesOut = total;
    return 0;
}
