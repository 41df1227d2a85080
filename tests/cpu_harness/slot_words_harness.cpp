/*
 * slot_words_harness.cpp -- host build (g++) of the per-slot key functions of libre_amd/csrc/vrc_core.h: the keys the
 * brick upload folds with atomicMax (vrc_slot_max_key, vrc_slot_min_key), their inverses, and the three questions the
 * marches ask of a word (vrc_mip_cannot_raise, _cannot_lower, _cannot_reach), for tests/test_slot_words_cpu.py.
 * TEST INFRASTRUCTURE ONLY, like mip_harness.cpp next to it.
 */
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/vrc_hip.h"
#include "../../libre_amd/csrc/vrc_tables.h"

extern "C" void slot_words_float_keys( const float* v, uint32_t count, uint32_t* maxKey, uint32_t* minKey, float* maxBack,
                                       float* minBack )
{
    for( uint32_t i = 0; i < count; ++i )
    {
        maxKey[i] = vrc_slot_max_key( v[i] );
        minKey[i] = vrc_slot_min_key( v[i] );
        maxBack[i] = vrc_slot_max_float( maxKey[i] );
        minBack[i] = vrc_slot_min_float( minKey[i] );
    }
}

extern "C" void slot_words_stored_keys( const uint32_t* stored, uint32_t count, uint32_t* minKey, uint32_t* minBack )
{
    for( uint32_t i = 0; i < count; ++i )
    {
        minKey[i] = vrc_slot_min_key( stored[i] );
        minBack[i] = vrc_slot_min_value( minKey[i] );
    }
}

namespace
{
enum
{
    RAISE = 0,
    LOWER = 1,
    REACH_MAX = 2,
    REACH_MIN = 3
};

template < bool TRILINEAR, typename ATLAS_T, typename M >
int ask( int question, uint32_t word, M m )
{
    switch( question )
    {
    case RAISE:
        return vrc_mip_cannot_raise< TRILINEAR, ATLAS_T >( word, m ) ? 1 : 0;
    case LOWER:
        return vrc_mip_cannot_lower< TRILINEAR, ATLAS_T >( word, m ) ? 1 : 0;
    case REACH_MAX:
        return vrc_mip_cannot_reach< VRC_FOLD_MAX, TRILINEAR, ATLAS_T >( word, m ) ? 1 : 0;
    case REACH_MIN:
        return vrc_mip_cannot_reach< VRC_FOLD_MIN, TRILINEAR, ATLAS_T >( word, m ) ? 1 : 0;
    }
    return -1;
}
} // namespace

/* an integer M: point samples of the 8- and 16-bit atlases */
extern "C" int slot_words_ask_integer( int question, uint32_t atlasBytes, uint32_t word, uint32_t m )
{
    if( atlasBytes == 1 )
        return ask< false, uint8_t >( question, word, m );
    if( atlasBytes == 2 )
        return ask< false, uint16_t >( question, word, m );
    return -1;
}

/* a float M: the float atlas (atlasBytes 4), and trilinear samples of the 8- and 16-bit atlases */
extern "C" int slot_words_ask_float( int question, uint32_t atlasBytes, int trilinear, uint32_t word, float m )
{
    if( atlasBytes == 4 )
        return trilinear ? ask< true, float >( question, word, m ) : ask< false, float >( question, word, m );
    if( atlasBytes == 2 )
        return trilinear ? ask< true, uint16_t >( question, word, m ) : ask< false, uint16_t >( question, word, m );
    if( atlasBytes == 1 )
        return trilinear ? ask< true, uint8_t >( question, word, m ) : ask< false, uint8_t >( question, word, m );
    return -1;
}
