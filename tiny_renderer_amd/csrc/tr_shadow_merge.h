// tr_shadow_merge.h -- the rule of merging two scenes' shadow buffers (k_shadow_merge, tr_shadow_merge_host): the
// reference's light-space pass is a running maximum, `if z_value >= shadow_buffer[index] { shadow_buffer[index] = z_value }`
// (shader.rs:703, 841), without culling, and both scenes of a composite share the shadow matrix (it depends on light,
// look_at, up and the frame size alone, shader.rs:234-255).  So the shadow buffer of the concatenated mesh A ++ B is A's
// buffer merged with B's by that same test, pixel by pixel:
//     if (zs >= zd) zd = zs
// bit for bit, the sign of a zero included: where the maximum is a zero and B holds a zero fragment, B's last one
// decides the sign in the concatenated pass as it does here (>= passes between +0.0 and -0.0); otherwise A's value
// stays.  A NaN on either side compares false and dst keeps its value, as a NaN fragment never enters the buffer.
// A pixel src never drew holds f32::MIN, which replaces nothing but another f32::MIN.  One function for the device and
// the host compiler, so that both see the same text.
#pragma once

#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

// The value dst's pixel holds after the merge: src's where the reference's test passes, else its own.
TR_HD float shadow_merge(float zs, float zd) { return (zs >= zd) ? zs : zd; }

// k_shadow_merge's arguments, passed by value.  Both buffers: index x + y * width, y up, the whole frame (a band scene's
// shadow buffer is full-frame too); the flags are the scenes' per-tile fast-clear flags over that grid (non-zero: every
// value of the tile is f32::MIN and its memory is stale).
struct ShadowMergeArgs {
    float *dst;
    uint32_t *dst_clean;
    const float *src;
    const uint32_t *src_clean;
    DevFrame frame;   // the whole frame (tr_scene::frame_full)
};

}  // namespace tr
