// tr_outline.h -- the rule of depth-edge outlines (k_outline, tr_outline_host, tr_outline_kinds): ink is laid over a
// finished colour frame where its own z buffer has a silhouette, a depth step or a fold.  Conventions as in tr_ao.h: z is
// indexed x + y * W, y up; a pixel is drawn when bits(z) != bits(f32::MIN); a larger z is nearer.  The 4-neighbours of p
// are (x +- 1, y) and (x, y +- 1); one outside the frame DOES NOT EXIST and contributes nothing (which is not the same
// as "not drawn": a model cut by the frame's border gets no ink there).
//   kinds  : of a drawn pixel p with depth z0 (a pixel that is not drawn has kind 0):
//              SIL = 1    some existing neighbour is not drawn
//              STEP = 2   some existing drawn neighbour q has fl(z0 - zq) > depth_step: the nearer side of a step only
//              CREASE = 4 (only with TR_OUTLINE_CREASES) on an axis, horizontal or vertical, whose two neighbours a and b
//                         both exist and are drawn:  fabsf(fl(z0 - za)) > depth_step is false, fabsf(fl(z0 - zb)) >
//                         depth_step is false, and fabsf(fl(fl(za + zb) - fl(z0 + z0))) > crease.  A plane at any tilt
//                         has second difference 0 up to rounding; a fold has not; a step is left to STEP.
//   seed   : p is a seed when its kinds are not 0.
//   ink    : p is inked when some q inside the frame with max(|dx|, |dy|) <= radius is a seed -- drawn or not.
//   output : base = paper under TR_OUTLINE_ONLY, else the stored colour F_p; an inked pixel gets, per channel,
//            (ink[c] * opacity + base[c] * (256 - opacity) + 128) >> 8, any other pixel base.
// Every f32 operation rounds once (the library is built with -ffp-contract=off); a comparison with a NaN is false, so a
// NaN depth seeds nothing by STEP or CREASE and is no step for its neighbours.  A pixel's output depends on the depths
// around it and on its own colour alone: the rule works in place.  One text for the device and the host compiler; only
// where the depths come from differs (k_outline: LDS, the host: the caller's array).
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr int OUTLINE_MAX_RADIUS = 3;        // (= TR_OUTLINE_MAX_RADIUS)
constexpr uint32_t OUTLINE_CREASES = 0x1u;   // (= TR_OUTLINE_CREASES)
constexpr uint32_t OUTLINE_ONLY = 0x2u;      // (= TR_OUTLINE_ONLY)
constexpr uint32_t OUTLINE_SIL = 1u, OUTLINE_STEP = 2u, OUTLINE_CREASE = 4u;

// The numbers of a call: ink and paper as packed pixels (r in bits 0..7, g in 8..15, b in 16..23).
struct OutlineRule {
    uint32_t radius, flags, opacity, ink, paper;
    float depth_step, crease;
};

TR_HD bool outline_drawn(float z) { return f32_bits(z) != TR_F32_MIN_BITS; }

// One neighbour q (which exists) of the drawn pixel with depth z0: the kinds it raises.
TR_HD uint32_t outline_neighbour(float z0, float zq, float depth_step)
{
    if (!outline_drawn(zq)) return OUTLINE_SIL;
    return z0 - zq > depth_step ? OUTLINE_STEP : 0u;
}

// One axis of the drawn pixel with depth z0 whose neighbours a and b both exist: CREASE or nothing.
TR_HD uint32_t outline_axis(float z0, float za, float zb, float depth_step, float crease)
{
    if (!outline_drawn(za) || !outline_drawn(zb)) return 0u;
    if (fabsf(z0 - za) > depth_step) return 0u;
    if (fabsf(z0 - zb) > depth_step) return 0u;
    return fabsf((za + zb) - (z0 + z0)) > crease ? OUTLINE_CREASE : 0u;
}

// The kinds of a pixel: its depth, the depths of its neighbours at x - 1, x + 1, y - 1, y + 1 and which of them exist
// (bits 0..3 of `exist`, in that order; the depth of one that does not exist is not looked at).
TR_HD uint32_t outline_kinds(float z0, float zl, float zr, float zd, float zu, uint32_t exist, const OutlineRule &q)
{
    if (!outline_drawn(z0)) return 0u;
    uint32_t k = 0u;
    if (exist & 1u) k |= outline_neighbour(z0, zl, q.depth_step);
    if (exist & 2u) k |= outline_neighbour(z0, zr, q.depth_step);
    if (exist & 4u) k |= outline_neighbour(z0, zd, q.depth_step);
    if (exist & 8u) k |= outline_neighbour(z0, zu, q.depth_step);
    if (q.flags & OUTLINE_CREASES) {
        if ((exist & 3u) == 3u) k |= outline_axis(z0, zl, zr, q.depth_step, q.crease);
        if ((exist & 12u) == 12u) k |= outline_axis(z0, zd, zu, q.depth_step, q.crease);
    }
    return k;
}

// Which neighbours of (x, y) exist in a frame of W x H pixels (the `exist` of outline_kinds).
TR_HD uint32_t outline_exist(int32_t x, int32_t y, int32_t W, int32_t H)
{
    return (x > 0 ? 1u : 0u) | (x + 1 < W ? 2u : 0u) | (y > 0 ? 4u : 0u) | (y + 1 < H ? 8u : 0u);
}

// One channel of an inked pixel.  (255 * 256 + 128 < 2^16.)
TR_HD uint32_t outline_channel(uint32_t ink, uint32_t base, uint32_t opacity)
{
    return (mul24(ink, opacity) + mul24(base, 256u - opacity) + 128u) >> 8;
}

// An inked pixel, packed.
TR_HD uint32_t outline_px(uint32_t base, const OutlineRule &q)
{
    return outline_channel(q.ink & 0xFFu, base & 0xFFu, q.opacity) |
           (outline_channel((q.ink >> 8) & 0xFFu, (base >> 8) & 0xFFu, q.opacity) << 8) |
           (outline_channel((q.ink >> 16) & 0xFFu, (base >> 16) & 0xFFu, q.opacity) << 16);
}

// The kinds of every pixel on the host (the body of tr_outline_kinds), in z's orientation.
inline void outline_kinds_host(uint32_t width, uint32_t height, const float *z, const OutlineRule &q, uint8_t *kinds)
{
    const int32_t W = (int32_t)width, H = (int32_t)height;
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const size_t at = (size_t)x + (size_t)y * (size_t)W;
            const uint32_t e = outline_exist(x, y, W, H);
            const float none = 0.0f;
            kinds[at] = (uint8_t)outline_kinds(z[at], (e & 1u) ? z[at - 1] : none, (e & 2u) ? z[at + 1] : none,
                                               (e & 4u) ? z[at - (size_t)W] : none, (e & 8u) ? z[at + (size_t)W] : none, e, q);
        }
}

// The rule over a whole frame on the host (the body of tr_outline_host; the caller has checked the parameters).  z: index
// x + y * width, y up; rgb and out: row 0 = top; out may be rgb.
inline void outline_host(uint32_t width, uint32_t height, const float *z, const uint8_t *rgb, uint8_t *out, const OutlineRule &q)
{
    const int64_t W = width, H = height, R = q.radius;
    std::vector<uint8_t> seed((size_t)(W * H)), wide((size_t)(W * H));
    outline_kinds_host(width, height, z, q, seed.data());
    // the square of the radius is a product: along the rows, then along the columns
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            uint8_t any = 0;
            for (int64_t qx = x - R < 0 ? 0 : x - R; qx <= x + R && qx < W; qx++) any |= seed[(size_t)(qx + y * W)];
            wide[(size_t)(x + y * W)] = any;
        }
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            uint8_t any = 0;
            for (int64_t qy = y - R < 0 ? 0 : y - R; qy <= y + R && qy < H; qy++) any |= wide[(size_t)(x + qy * W)];
            const size_t ci = (size_t)((H - 1 - y) * W + x) * 3u;
            const uint32_t base = (q.flags & OUTLINE_ONLY) ? q.paper : (uint32_t)rgb[ci] | ((uint32_t)rgb[ci + 1] << 8) | ((uint32_t)rgb[ci + 2] << 16);
            const uint32_t o = any ? outline_px(base, q) : base;
            out[ci] = (uint8_t)(o & 0xFFu), out[ci + 1] = (uint8_t)((o >> 8) & 0xFFu), out[ci + 2] = (uint8_t)((o >> 16) & 0xFFu);
        }
}

// k_outline's arguments, passed by value.  z: index x + y * width, y up; fb and out: rgb8, buffer row height - 1 - y; out
// is fb (in place) or does not overlap it.  zclean / fbclean: the scene's per-tile fast-clear flags over the whole
// frame's tile grid (band scenes are refused); in place the kernel lowers the colour flag of a flagged tile it writes.
struct OutlineArgs {
    const float *z;
    const uint32_t *zclean;
    const uint8_t *fb;
    uint32_t *fbclean;
    uint8_t *out;
    DevFrame frame;
    OutlineRule rule;
};

}  // namespace tr
