/* Stand-alone program for the AddressSanitizer / UBSan run of the tile culling's host build
 * (tests/test_tile_cull_cpu.py::test_stand_alone_program_under_sanitizers).  TEST INFRASTRUCTURE ONLY.
 * argv[1..]: scenes as the test writes them (a header of 16 uint32 words, then view, render data, clip planes, transfer
 * function, row map, node list, row-major atlas).  For each: the masks and the per-ray statement of every tile, then the
 * frame with the candidates and with candidates = nullptr -- the wave's array is a heap block of exactly
 * VRC_TILE_CANDIDATES entries, so a store or a read past it is an error here. */
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../cpu_harness/cull_harness.cpp"

namespace
{
bool read_exact( std::FILE* f, void* to, size_t n ) { return n == 0 || std::fread( to, 1, n, f ) == n; }

int run( const char* path )
{
    std::FILE* f = std::fopen( path, "rb" );
    if( !f )
        return 1;
    uint32_t h[16];
    vrc_view_data view;
    vrc_render_data render;
    int rc = 1;
    if( read_exact( f, h, sizeof( h ) ) && h[0] == 0x4C4C5543u && h[13] == sizeof( view ) && h[14] == sizeof( vrc_node_data ) &&
        h[15] == sizeof( render ) && read_exact( f, &view, sizeof( view ) ) && read_exact( f, &render, sizeof( render ) ) )
    {
        const uint32_t voxelBytes = h[1], *atlasDim = h + 2, *slotDim = h + 5, W = h[8], H = h[9], nPlanes = h[10], nNodes = h[11],
                       nRows = h[12];
        std::vector< float > planes( 4u * nPlanes ), tf( 4u * 256u );
        std::vector< uint32_t > rows( nRows );
        std::vector< vrc_node_data > nodes( nNodes );
        std::vector< uint8_t > atlas( (size_t)voxelBytes * atlasDim[0] * atlasDim[1] * atlasDim[2] );
        if( read_exact( f, planes.data(), planes.size() * 4u ) && read_exact( f, tf.data(), tf.size() * 4u ) &&
            read_exact( f, rows.data(), rows.size() * 4u ) && read_exact( f, nodes.data(), nodes.size() * sizeof( vrc_node_data ) ) &&
            read_exact( f, atlas.data(), atlas.size() ) )
        {
            const uint32_t* const rowMap = nRows ? rows.data() : nullptr;
            const uint32_t nTiles = ( ( W + CULL_TILE_W - 1u ) / CULL_TILE_W ) * ( ( H + CULL_TILE_H - 1u ) / CULL_TILE_H );
            std::vector< uint8_t > kept( (size_t)nTiles * nNodes ), needed( (size_t)nTiles * nNodes );
            std::vector< uint32_t > counts( nTiles );
            std::vector< int32_t > regimes( nTiles );
            rc = cull_tile_masks( atlasDim, slotDim, W, H, planes.data(), nPlanes, &view, nNodes, nodes.data(), &render, rowMap, 0, 0,
                                  0, nullptr, 0, kept.data(), counts.data(), regimes.data() );
            rc = rc ? rc : cull_needed( atlasDim, slotDim, W, H, planes.data(), nPlanes, &view, nNodes, nodes.data(), &render, rowMap, 0,
                                        0, 0, nullptr, 0, needed.data() );
            size_t dropped = 0;
            for( size_t i = 0; i < kept.size(); ++i )
                dropped += ( needed[i] && !kept[i] ) ? 1u : 0u;
            std::vector< float > a( (size_t)W * H * 4u, 0.0f ), b( a );
            uint64_t na = 0, nb = 0;
            for( int mode = voxelBytes == 1 ? 0 : 1; mode <= 4 && !rc; ++mode )
            {
                std::fill( a.begin(), a.end(), 0.0f );
                std::fill( b.begin(), b.end(), 0.0f );
                rc = cull_render( atlas.data(), voxelBytes, atlasDim, slotDim, a.data(), W, H, planes.data(), nPlanes, tf.data(), &view,
                                  nNodes, nodes.data(), &render, rowMap, 0, 0, 0, nullptr, 0, mode, 0.25f, 1, &na, regimes.data() );
                rc = rc ? rc : cull_render( atlas.data(), voxelBytes, atlasDim, slotDim, b.data(), W, H, planes.data(), nPlanes, tf.data(),
                                            &view, nNodes, nodes.data(), &render, rowMap, 0, 0, 0, nullptr, 0, mode, 0.25f, 0, &nb, nullptr );
                if( !rc && ( std::memcmp( a.data(), b.data(), a.size() * 4u ) != 0 || na != nb ) )
                    rc = 10 + mode;
            }
            const std::string p( path );
            std::printf( "%s: regime %d, %u tiles, %u entries, dropped %zu, samples %llu, equal %d\n",
                         p.substr( p.find_last_of( '/' ) + 1 ).c_str(), (int)regimes[0], nTiles, nNodes, dropped,
                         (unsigned long long)na, rc == 0 ? 1 : 0 );
            if( dropped )
                rc = 9;
        }
    }
    std::fclose( f );
    return rc;
}
} // namespace

int main( int argc, char** argv )
{
    for( int i = 1; i < argc; ++i )
        if( const int rc = run( argv[i] ) )
        {
            std::printf( "%s: failed (%d)\n", argv[i], rc );
            return 1;
        }
    std::printf( "DONE\n" );
    return 0;
}
