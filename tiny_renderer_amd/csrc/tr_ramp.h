// tr_ramp.h -- the rule of the depth ramp (k_ramp, tr_ramp_host, tr_ramp_positions): every pixel of a finished colour
// frame is blended with an entry of a 1-D table of n rgba8 colours, n = 2..1024, chosen by the pixel's own depth.  Entry k
// is table[4 k .. 4 k + 3] = r, g, b, a.  For a pixel with depth z (what tr_scene_read_z_f32 returns: index x + y * W, y
// up) and stored colour d:
//   position : bits(z) == bits(f32::MIN): the pixel is not drawn, takes no position and the parameters' own `undrawn`
//              entry (r in bits 0..7, g 8..15, b 16..23, alpha 24..31).  Otherwise p = (fl(fl(z - z0) * scale)) as u32,
//              every f32 operation rounded once; `as u32` is Rust's cast (f32_to_u32, tr_math.h): truncating, saturating,
//              NaN and negatives give 0.  p counts 1/256 of a table step; scale may be negative (nearer is larger here,
//              so a ramp that grows with distance has scale < 0).  With pmax = (n - 1) * 256: p = min(p, pmax), or with
//              RAMP_REPEAT p = p % pmax.  i = p >> 8, f = p & 255, j = min(i + 1, n - 1).
//   entry    : per channel c of r, g, b, a: e_c = (E_i[c] * (256 - f) + E_j[c] * f + 128) >> 8.  The sum is at most
//              255 * 256 + 128 < 2^16, so two channels are summed in the two halves of one word without a carry.
//   blend    : coverage cov = e_a * opacity, opacity 0..256: 0..65280; the output is tr_layer.h's layer_px<mode>(e, d, cov)
//              -- its seven modes, its two exact divisions.  A pixel that is not drawn blends `undrawn` the same way.
// It follows: cov == 0 leaves d; cov == 65280 under NORMAL gives the entry's colour exactly (a depth view); f == 0 gives
// E_i exactly, so p == pmax gives the last entry; a clamped j (i == n - 1) goes with f == 0 and carries weight 0.  A pixel
// depends on itself alone: the rule works in place.  Only colour changes.  One text for the device and the host compiler;
// only where the table lives differs (k_ramp: LDS, one word an entry; the host: a vector of such words).
#pragma once

#include <stdint.h>

#include <vector>

#include "tr_layer.h"
#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t RAMP_MAX_N = 1024u;  // (= TR_RAMP_MAX_N) 4 KB of LDS
constexpr uint32_t RAMP_REPEAT = 0x1u;  // (= TR_RAMP_REPEAT)
constexpr uint32_t RAMP_NO_POSITION = 0xFFFFFFFFu;  // tr_ramp_positions: the depth is not drawn

static_assert(255u * 256u + 128u < (1u << 16), "an interpolated channel's sum fits a u16: two share a word without a carry");
static_assert((RAMP_MAX_N - 1u) * 256u < (1u << 24), "pmax fits mul24 and a table index stays below n");

// The numbers of a call: the header's tr_ramp_params with the table's length beside them.
struct RampRule {
    float z0, scale;
    uint32_t mode, opacity, undrawn, flags, n;
};

// The position of a drawn pixel with depth z, in 1/256 of a table step: 0 .. (n - 1) * 256.
TR_HD uint32_t ramp_position(float z, const RampRule &q)
{
    const float d = z - q.z0;
    const float c = d * q.scale;
    const uint32_t p = f32_to_u32(c);
    const uint32_t pmax = (q.n - 1u) << 8;
    if (q.flags & RAMP_REPEAT) return p % pmax;
    return p < pmax ? p : pmax;
}

// The table's entry at position p (<= pmax), interpolated: red and blue in the halves of one word, green and alpha in
// those of another.  table: n packed entries, wherever they live.
TR_HD uint32_t ramp_entry(const uint32_t *table, uint32_t n, uint32_t p)
{
    const uint32_t i = p >> 8, f = p & 255u, j = i + 1u < n ? i + 1u : n - 1u;
    const uint32_t ei = table[i], ej = table[j];
    const uint32_t rb = mul24(ei & 0x00FF00FFu, 256u - f) + mul24(ej & 0x00FF00FFu, f) + 0x00800080u;
    const uint32_t ga = mul24((ei >> 8) & 0x00FF00FFu, 256u - f) + mul24((ej >> 8) & 0x00FF00FFu, f) + 0x00800080u;
    return ((rb >> 8) & 0x00FF00FFu) | (ga & 0xFF00FF00u);
}

// What a pixel with depth z blends: the interpolated entry, or `undrawn`.
TR_HD uint32_t ramp_source(const uint32_t *table, float z, const RampRule &q)
{
    const uint32_t e = ramp_entry(table, q.n, ramp_position(z, q));
    return layer_drawn(z) ? e : q.undrawn;
}

// The coverage of a source pixel e (alpha in bits 24..31).
TR_HD uint32_t ramp_coverage(uint32_t e, uint32_t opacity) { return mul24(e >> 24, opacity); }

// Does a logically cleared frame -- `undrawn` over black everywhere -- stay black?
TR_HD bool ramp_keeps_cleared_black(const RampRule &q)
{
    return layer_px_by(q.mode, q.undrawn, 0u, ramp_coverage(q.undrawn, q.opacity)) == 0u;
}

// The caller's table (4 n bytes) as the packed entries the rule reads.
inline void ramp_expand(uint32_t n, const uint8_t *rgba, uint32_t *words)
{
    for (uint32_t k = 0; k < n; k++)
        words[k] = (uint32_t)rgba[4 * k] | ((uint32_t)rgba[4 * k + 1] << 8) | ((uint32_t)rgba[4 * k + 2] << 16) | ((uint32_t)rgba[4 * k + 3] << 24);
}

// The rule over a whole frame on the host (the body of tr_ramp_host; the caller has checked the parameters).  rgb and
// out: W x H rgb8, row 0 = top; out may be rgb; z: index x + y * W, y up.
inline void ramp_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const RampRule &q, const uint8_t *table, uint8_t *out)
{
    std::vector<uint32_t> words(q.n);
    ramp_expand(q.n, table, words.data());
    const size_t W = width, H = height;
    for (size_t r = 0; r < H; r++)
        for (size_t x = 0; x < W; x++) {
            const uint8_t *sp = rgb + (r * W + x) * 3;
            uint8_t *o = out + (r * W + x) * 3;
            const uint32_t d = (uint32_t)sp[0] | ((uint32_t)sp[1] << 8) | ((uint32_t)sp[2] << 16);
            const uint32_t e = ramp_source(words.data(), z[x + (H - 1 - r) * W], q);
            const uint32_t v = layer_px_by(q.mode, e, d, ramp_coverage(e, q.opacity));
            o[0] = (uint8_t)(v & 0xFFu), o[1] = (uint8_t)((v >> 8) & 0xFFu), o[2] = (uint8_t)((v >> 16) & 0xFFu);
        }
}

// k_ramp's arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y; out is fb (in place) or does not
// overlap it, at any byte address.  fbclean / zclean: the frame's per-tile colour and z fast-clear flags over its 128 x 16
// tile grid (fbclean may be null: nothing is known).  z: the frame's depth, y up.  lower: null, or fbclean again -- in
// place a flagged tile that is stored whole has its flag lowered.  table: rule.n packed entries in device memory, padded
// to whole 16-byte pieces.
struct RampArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *lower;
    const float *z;
    const uint32_t *zclean;
    const uint32_t *table;
    DevFrame frame;
    RampRule rule;
};

}  // namespace tr
