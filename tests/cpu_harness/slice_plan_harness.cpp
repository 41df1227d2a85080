/*
 * slice_plan_harness.cpp -- vrc_plan_mode (libre_amd/csrc/vrc_plan.h) asked about a slice frame, for
 * tests/test_slice_cpu.py.  TEST INFRASTRUCTURE ONLY.  render_plan_harness.cpp holds the function to the text it
 * replaced over the inputs that text knew; this one calls it with the two inputs the slice added.
 */
#include <cstdint>
#include <cstring>

#include "../../libre_amd/csrc/vrc_plan.h"

/* One call.  opts: projection, kernel, variant, filter, shading, compositeDepth, preint, mipDepth.  latchProjection: -1 =
 * the frame's first pass.  latchedPlane: the plane the frame's first slice pass took, or null.  plane: vrc_set_slice's,
 * or null where it was never called.  out: slice, mip, shade, cdepth, preint, classify, linear, plain.  msg: the
 * refusal's text (empty: served).  Returns the code */
extern "C" int slice_plan_mode( const int64_t opts[8], int rayLod, int64_t latchProjection, const float* latchedPlane,
                                const float* plane, uint32_t elemBytes, int32_t out[8], char* msg, uint32_t msgBytes )
{
    vrc_options o;
    o.projection = opts[0];
    o.kernel = opts[1];
    o.variant = opts[2];
    o.filter = opts[3];
    o.shading = opts[4];
    o.compositeDepth = opts[5];
    o.preint = opts[6];
    o.mipDepth = opts[7];
    vrc_latches l;
    l.projection = latchProjection;
    if( latchedPlane )
    {
        l.slice = true;
        for( int i = 0; i < 4; ++i )
            l.slicePlane[i] = latchedPlane[i];
    }
    vrc_mode m;
    const vrc_refusal r = vrc_plan_mode( o, l, rayLod != 0, false, 0.0f, 0.0f, elemBytes, m, plane != nullptr, plane );
    const bool flags[8] = { m.slice, m.mip, m.shade, m.cdepth, m.preint, m.classify, m.linear, m.plain() };
    for( int i = 0; i < 8; ++i )
        out[i] = flags[i] ? 1 : 0;
    if( msg && msgBytes )
    {
        std::strncpy( msg, r.msg ? r.msg : "", msgBytes - 1u );
        msg[msgBytes - 1u] = 0;
    }
    return r.code;
}
