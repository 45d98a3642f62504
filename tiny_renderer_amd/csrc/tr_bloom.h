// tr_bloom.h -- the rule of bloom (k_bloom, tr_bloom_host): the highlights of a finished colour frame are keyed out,
// blurred by a fixed tent of radius R and added back.  Over the stored u8 values F of the frame; a pixel outside the
// frame is black:
//   key   : m = max(F_p[0], F_p[1], F_p[2]);  B_p[c] = (m > threshold) ? F_p[c] : 0
//   tent  : w(d) = R + 1 - |d| for |d| <= R;  S = (R + 1)^2 is the sum of the weights of one axis;  D = S^2
//   blur  : V_p[c] = sum over |dx| <= R, |dy| <= R of w(dx) * w(dy) * B_(x + dx, y + dy)[c]
//           The kernel is a product: a horizontal pass Hh = sum of w(dx) * B followed by a vertical pass
//           V = sum of w(dy) * Hh gives the same integers in any order.  With R <= 15, Hh <= 255 * 256 fits a u16 and
//           V <= 255 * 65536 fits a u32.
//   glow  : G_p[c] = (V_p[c] + D / 2) / D                                  (integer division, rounded once)
//   out   : min(255, F_p[c] + ((strength * G_p[c] + 128) >> 8));  TR_BLOOM_GLOW_ONLY: G_p[c], strength is not used
// Everything is integer: the order of the taps does not matter.  One text for the device and the host compiler; only
// where B and Hh live differs (k_bloom: LDS, the host: arrays of the frame's size).
#pragma once

#include <stdint.h>

#include <vector>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr int BLOOM_MAX_RADIUS = 15;         // (= TR_BLOOM_MAX_RADIUS)
constexpr uint32_t BLOOM_GLOW_ONLY = 1u;     // (= TR_BLOOM_GLOW_ONLY)
constexpr uint32_t BLOOM_MAX_STRENGTH = 1024u;

// One axis: S = (R + 1)^2 <= 256, so Hh <= 255 * 256 = 65280 < 2^16 -- two channels share a word without a carry.  Both
// axes: V + D / 2 <= 255 * 65536 + 32768 = 16,744,448 < 2^24.  strength * G + 128 <= 1024 * 255 + 128 < 2^19.
static_assert(255u * (BLOOM_MAX_RADIUS + 1) * (BLOOM_MAX_RADIUS + 1) < (1u << 16), "a horizontal sum fits a u16");
static_assert(255ull * 65536ull + 32768ull < (1ull << 32) && (BLOOM_MAX_RADIUS + 1) * (BLOOM_MAX_RADIUS + 1) == 256, "a sum of both axes fits a u32");

// The numbers of a call.
struct BloomRule {
    uint32_t radius, threshold, strength, glow_only;
};

// A pixel as the passes see it: r in bits 0..7, g in 8..15, b in 16..23.
TR_HD uint32_t bloom_pack(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// key: the packed pixel, or 0 where its largest channel does not exceed the threshold.
TR_HD uint32_t bloom_key(uint32_t px, uint32_t threshold)
{
    const uint32_t r = px & 0xFFu, g = (px >> 8) & 0xFFu, b = (px >> 16) & 0xFFu;
    const uint32_t m = r > g ? (r > b ? r : b) : (g > b ? g : b);
    return m > threshold ? px : 0u;
}

// tent: w(d), |d| <= R.
TR_HD uint32_t bloom_weight(int32_t R, int32_t d) { return (uint32_t)(R + 1 - (d < 0 ? -d : d)); }

// S and D of a radius.
TR_HD uint32_t bloom_divisor(uint32_t R) { return (R + 1u) * (R + 1u) * (R + 1u) * (R + 1u); }

// The horizontal sums of a pixel: r in the low and b in the high half of rb (neither exceeds 65280), g in g.
struct BloomH {
    uint32_t rb, g;
};

// One horizontal tap: the keyed packed pixel `px` under weight w.  (Both factors are below 2^24: mul24, one full-rate
// instruction on the device, the plain product on the host.)
TR_HD void bloom_h_tap(BloomH &h, uint32_t px, uint32_t w)
{
    h.rb += mul24(px & 0x00FF00FFu, w);
    h.g += mul24((px >> 8) & 0xFFu, w);
}

// The sums of both axes of a pixel.
struct BloomV {
    uint32_t r, g, b;
};

// One vertical tap: the horizontal sums `h` of the pixel above or below under weight w.
TR_HD void bloom_v_tap(BloomV &v, const BloomH &h, uint32_t w)
{
    v.r += mul24(h.rb & 0xFFFFu, w);
    v.g += mul24(h.g, w);
    v.b += mul24(h.rb >> 16, w);
}

// glow: one channel.
TR_HD uint32_t bloom_glow(uint32_t V, uint32_t D) { return (V + D / 2u) / D; }

// glow: the pixel, packed.
TR_HD uint32_t bloom_glow_px(const BloomV &v, uint32_t D) { return bloom_pack(bloom_glow(v.r, D), bloom_glow(v.g, D), bloom_glow(v.b, D)); }

// out: one channel of the frame F and of the glow G.
TR_HD uint32_t bloom_add(uint32_t F, uint32_t G, uint32_t strength)
{
    const uint32_t s = F + ((mul24(strength, G) + 128u) >> 8);
    return s < 255u ? s : 255u;
}

// out: the finished pixel from the packed frame pixel and the packed glow.
TR_HD uint32_t bloom_out_px(uint32_t f, uint32_t g, const BloomRule &q)
{
    if (q.glow_only != 0u) return g;
    return bloom_pack(bloom_add(f & 0xFFu, g & 0xFFu, q.strength), bloom_add((f >> 8) & 0xFFu, (g >> 8) & 0xFFu, q.strength),
                      bloom_add((f >> 16) & 0xFFu, (g >> 16) & 0xFFu, q.strength));
}

// The rule over a whole frame on the host (the body of tr_bloom_host; the caller has checked the parameters), by the two
// passes of the kernel.  rgb and out: row 0 = top, out != rgb.  Reads 3 * width * height bytes, writes as many.
inline void bloom_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out, const BloomRule &q)
{
    const int64_t W = width, H = height, R = q.radius;
    const uint32_t D = bloom_divisor(q.radius);
    std::vector<uint32_t> key((size_t)(W * H));
    std::vector<BloomH> hh((size_t)(W * H));
    for (int64_t i = 0; i < W * H; i++) key[(size_t)i] = bloom_key(bloom_pack(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]), q.threshold);
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            BloomH h = { 0u, 0u };
            for (int64_t dx = -R; dx <= R; dx++)
                if (x + dx >= 0 && x + dx < W) bloom_h_tap(h, key[(size_t)(y * W + x + dx)], bloom_weight((int32_t)R, (int32_t)dx));
            hh[(size_t)(y * W + x)] = h;
        }
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            BloomV v = { 0u, 0u, 0u };
            for (int64_t dy = -R; dy <= R; dy++)
                if (y + dy >= 0 && y + dy < H) bloom_v_tap(v, hh[(size_t)((y + dy) * W + x)], bloom_weight((int32_t)R, (int32_t)dy));
            const int64_t i = y * W + x;
            const uint32_t o = bloom_out_px(bloom_pack(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]), bloom_glow_px(v, D), q);
            out[3 * i] = (uint8_t)(o & 0xFFu), out[3 * i + 1] = (uint8_t)((o >> 8) & 0xFFu), out[3 * i + 2] = (uint8_t)((o >> 16) & 0xFFu);
        }
}

// k_bloom's arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y, out does not overlap fb; fbclean:
// the scene's per-tile colour fast-clear flags over the whole frame's tile grid (band scenes are refused; may be null:
// nothing is known about the colour); out_clean: null, or where the workgroup writes the flag of its tile of `out`.
struct BloomArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *out_clean;
    DevFrame frame;
    BloomRule rule;
};

}  // namespace tr
