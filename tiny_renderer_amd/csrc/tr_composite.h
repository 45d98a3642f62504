// tr_composite.h -- the rule of depth compositing (k_composite, tr_composite_host): one scene's frame (src) is merged
// into another's (dst) pixel by pixel by the reference's own depth test, `if z_value <= z_buffer[index] { return false }`
// (shader.rs:175).  With zs, zd the two z values of a pixel:
//     covered = bits(zs) != bits(f32::MIN)   -- a pixel still at the cleared value was never drawn; a drawn pixel cannot
//                                               hold that value, since a fragment at f32::MIN fails the test against it
//     wins    = covered && !(zs <= zd)       -- the reference's test: a NaN on either side compares false, so it passes
// Where src wins, dst takes src's colour, z and (winner + winner_base, wrapping); elsewhere dst keeps its own -- ties
// too, so the order of the calls is the tie order, as the polygon order is inside one scene.  One function for the
// device and the host compiler, so that both see the same text.
#pragma once

#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

// Does src's fragment at depth zs replace dst's at depth zd?
TR_HD bool composite_wins(float zs, float zd)
{
    const bool covered = f32_bits(zs) != TR_F32_MIN_BITS;
    return covered && !(zs <= zd);
}

// The winner word dst takes from a winning src pixel.
TR_HD uint32_t composite_winner(uint32_t src_winner, uint32_t winner_base) { return src_winner + winner_base; }

// k_composite's arguments, passed by value.  z and winner words: index x + y * width, y up; colour: rgb8, buffer row
// height - 1 - y.  The *_zclean / dst_fbclean flags are the scenes' per-tile fast-clear flags over dst's band grid.
struct CompositeArgs {
    float *dst_z;
    uint8_t *dst_fb;
    uint32_t *dst_winner;         // null: dst has no winner tap
    uint32_t *dst_zclean;
    uint32_t *dst_fbclean;
    const float *src_z;
    const uint8_t *src_fb;
    const uint32_t *src_winner;   // read only where dst_winner is not null
    const uint32_t *src_zclean;
    DevFrame frame;
    uint32_t winner_base;
};

}  // namespace tr
