// tr_dof.h -- the rule of depth of field (k_dof, tr_dof_host): a finished colour frame is blurred by its own z buffer.
//   circle  : the circle of confusion of a pixel with depth z (what tr_scene_read_z_f32 returns):
//                 bits(z) == bits(f32::MIN), not drawn : coc = background_radius
//                 otherwise : coc = min(max_radius, (fl(fl(fl(|fl(z - focus)|) - range) * scale)) as u32)
//             `as u32` is Rust's cast (f32_to_u32, tr_math.h): truncating, saturating, NaN and negatives give 0.  So a
//             NaN z gives 0 and an infinite one max_radius.
//   weights : wt[r] = 32768 / ((2r + 1) * (2r + 1)), integer division, r = 0..8:
//             32768, 3640, 1310, 668, 404, 270, 193, 145, 113.
//   pixel   : with R = max_radius, the output at p = (x, y), per channel c, over the stored u8 values F:
//                 sw = 0, sc = 0
//                 for every q = (x + dx, y + dy), |dx| <= R, |dy| <= R, q inside the frame, max(|dx|, |dy|) <= coc(q):
//                     sw += wt[coc(q)];  sc += wt[coc(q)] * F_q[c]
//                 out_p[c] = (sc + sw / 2) / sw                       (u32 integer arithmetic)
//             Scatter written as gather: a pixel spreads over the square of its own circle with a weight inverse to
//             that square's area.  q = p always qualifies, so sw >= 113; pixels that are not drawn take part with their
//             stored colour and background_radius.  The sums are integers: the order of the taps does not matter.
//   TR_DOF_SHOW_COC : every pixel is coc(p) * 255 / max_radius in all three channels, integer division.
// Every f32 operation rounds once (the library is built with -ffp-contract=off).  One text for the device and the host
// compiler; only where coc(q) and F_q come from differs (k_dof: packed words in LDS, the host: the caller's arrays).
#pragma once

#include <math.h>
#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr int DOF_MAX_RADIUS = 8;        // (= TR_DOF_MAX_RADIUS)
constexpr uint32_t DOF_SHOW_COC = 1u;    // (= TR_DOF_SHOW_COC)
constexpr uint32_t DOF_UNIT = 32768u;    // the weight of a circle of radius 0

#define TR_DOF_WT(r) (32768u / ((2u * (r) + 1u) * (2u * (r) + 1u)))
static_assert(TR_DOF_WT(0) == 32768u && TR_DOF_WT(1) == 3640u && TR_DOF_WT(2) == 1310u && TR_DOF_WT(3) == 668u &&
                  TR_DOF_WT(4) == 404u && TR_DOF_WT(5) == 270u && TR_DOF_WT(6) == 193u && TR_DOF_WT(7) == 145u && TR_DOF_WT(8) == 113u,
              "the weight table of the rule");
// At most (2 * 8 + 1)^2 = 289 taps of weight <= 32768 over bytes <= 255: sc <= 289 * 32768 * 255 = 2,414,837,760 and
// sw / 2 <= 289 * 16384 = 4,734,976; their sum 2,419,572,736 < 2^32 = 4,294,967,296: u32 never overflows.  sw itself
// <= 289 * 32768 = 9,469,952 < 2^24.
static_assert((uint64_t)(2 * DOF_MAX_RADIUS + 1) * (2 * DOF_MAX_RADIUS + 1) * 32768u * 255u +
                      (uint64_t)(2 * DOF_MAX_RADIUS + 1) * (2 * DOF_MAX_RADIUS + 1) * 16384u < (1ull << 32),
              "the sums of a pixel fit u32");
static_assert((uint64_t)(2 * DOF_MAX_RADIUS + 1) * (2 * DOF_MAX_RADIUS + 1) * 32768u < (1ull << 24), "sw is exact as f32 and fits mul24");

// wt[coc], coc <= DOF_MAX_RADIUS: a chain of selects over constants (no table in memory on the device).
TR_HD uint32_t dof_weight(uint32_t coc)
{
    return coc == 0u ? TR_DOF_WT(0) : coc == 1u ? TR_DOF_WT(1) : coc == 2u ? TR_DOF_WT(2) : coc == 3u ? TR_DOF_WT(3)
         : coc == 4u ? TR_DOF_WT(4) : coc == 5u ? TR_DOF_WT(5) : coc == 6u ? TR_DOF_WT(6) : coc == 7u ? TR_DOF_WT(7)
                                                                                                       : TR_DOF_WT(8);
}

// The numbers of a call the circle needs.
struct DofRule {
    float focus, range, scale;
    uint32_t max_radius, background_radius;
};

// The circle of confusion of a pixel with depth z.
TR_HD uint32_t dof_coc(float z, const DofRule &q)
{
    if (f32_bits(z) == TR_F32_MIN_BITS) return q.background_radius;
    const float d = z - q.focus;
    const float a = fabsf(d);
    const float b = a - q.range;
    const float c = b * q.scale;
    const uint32_t u = f32_to_u32(c);
    return u < q.max_radius ? u : q.max_radius;
}

// TR_DOF_SHOW_COC: the value of all three channels.
TR_HD uint32_t dof_show(uint32_t coc, uint32_t max_radius) { return coc * 255u / max_radius; }

// A pixel as a tap sees it: colour in bits 0..23 (r lowest), circle in the top byte.  `packed >= (dist << 24)` is
// `dist <= coc`.
TR_HD uint32_t dof_pack(uint32_t r, uint32_t g, uint32_t b, uint32_t coc) { return r | (g << 8) | (b << 16) | (coc << 24); }

// The sums of a pixel: sw, and sc per channel.
struct DofSums {
    uint32_t w, r, g, b;
};

// One tap at distance dist = max(|dx|, |dy|): the packed pixel q and its weight wt[coc(q)].
TR_HD void dof_tap(DofSums &s, uint32_t packed, uint32_t wt, uint32_t dist)
{
    const uint32_t w = packed >= (dist << 24) ? wt : 0u;
    s.w += w;
    s.r += mul24(w, packed & 0xFFu);
    s.g += mul24(w, (packed >> 8) & 0xFFu);
    s.b += mul24(w, (packed >> 16) & 0xFFu);
}

// (n + 0) / sw for n = sc + sw / 2, exactly, with 113 <= sw < 2^24 and n <= 255 * sw + sw / 2 < 2^32, so the quotient is
// at most 255.  inv = fl(1 / fl(sw)) (sw is exact as f32).  q0 = trunc(fl(fl(n) * inv)): fl(n) has relative error
// <= 2^-24, inv <= 2^-24, the product <= 2^-24, together below 2^-22; the true quotient is below 256, so q0's argument is
// within 256 * 2^-22 = 2^-14 of it and q0 is floor(n / sw) - 1, floor(n / sw) or floor(n / sw) + 1.  One step either way
// on the exact remainder n - q0 * sw (|.| < 2 * sw < 2^25: it fits i32, q0 * sw <= 256 * sw < 2^32 and both factors fit
// mul24) gives floor(n / sw).
TR_HD uint32_t dof_div(uint32_t n, uint32_t sw, float inv)
{
    uint32_t q = f32_to_u32((float)n * inv);
    const int32_t rem = (int32_t)(n - mul24(q, sw));
    if (rem < 0) q -= 1u;
    else if (rem >= (int32_t)sw) q += 1u;
    return q;
}

// The finished pixel, packed like dof_pack with a zero top byte.
TR_HD uint32_t dof_finish(const DofSums &s)
{
    const float inv = 1.0f / (float)s.w;
    const uint32_t half = s.w >> 1;
    return dof_div(s.r + half, s.w, inv) | (dof_div(s.g + half, s.w, inv) << 8) | (dof_div(s.b + half, s.w, inv) << 16);
}

// The circles of n depths (the body of tr_dof_coc).  Reads n floats, writes n bytes.
inline void dof_coc_host(const DofRule &q, uint32_t n, const float *z, uint8_t *coc)
{
    for (uint32_t i = 0; i < n; i++) coc[i] = (uint8_t)dof_coc(z[i], q);
}

// The rule over a whole frame on the host (the body of tr_dof_host; the caller has checked the parameters).  z: index
// x + y * width, y up; rgb and out: row 0 = top, out != rgb.  Reads width * height floats and 3 * width * height bytes,
// writes 3 * width * height bytes, nothing else.
inline void dof_host(uint32_t width, uint32_t height, const float *z, const uint8_t *rgb, uint8_t *out, const DofRule &q, bool show_coc)
{
    const int64_t W = width, H = height, R = q.max_radius;
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            uint8_t *o = out + ((H - 1 - y) * W + x) * 3;
            if (show_coc) {
                o[0] = o[1] = o[2] = (uint8_t)dof_show(dof_coc(z[x + y * W], q), q.max_radius);
                continue;
            }
            DofSums s = { 0u, 0u, 0u, 0u };
            for (int64_t dy = -R; dy <= R; dy++)
                for (int64_t dx = -R; dx <= R; dx++) {
                    const int64_t qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const uint32_t coc = dof_coc(z[qx + qy * W], q);
                    const uint8_t *c = rgb + ((H - 1 - qy) * W + qx) * 3;
                    const int64_t ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
                    dof_tap(s, dof_pack(c[0], c[1], c[2], coc), dof_weight(coc), (uint32_t)(ax > ay ? ax : ay));
                }
            const uint32_t v = dof_finish(s);
            o[0] = (uint8_t)(v & 0xFFu), o[1] = (uint8_t)((v >> 8) & 0xFFu), o[2] = (uint8_t)((v >> 16) & 0xFFu);
        }
}

// k_dof's arguments, passed by value.  z: index x + y * width, y up; fb and out: rgb8, buffer row height - 1 - y, out
// does not overlap fb; zclean / fbclean: the scene's per-tile fast-clear flags over the whole frame's tile grid (band
// scenes are refused; fbclean may be null: nothing is known about the colour); out_clean: null, or where the workgroup
// writes the flag of its tile of `out`.
struct DofArgs {
    const float *z;
    const uint32_t *zclean;
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *out_clean;
    DevFrame frame;
    uint32_t show_coc;
    DofRule rule;
};

}  // namespace tr
