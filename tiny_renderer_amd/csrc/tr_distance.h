// tr_distance.h -- the rule of the distance field (k_dist_mask, k_dist_row, k_dist, k_dist_apply, tr_distance_host,
// tr_distance_ramp_host): for every pixel of a finished frame the SQUARED Euclidean distance, in pixels, to the nearest
// seed of the frame, capped at a radius R = 1..255, as a u16; and that field coloured through the scene's ramp table.
//   seeds : DIST_SEED_DRAWN: bits(z) != bits(f32::MIN) (layer_drawn, what the depth ramp calls drawn); DIST_SEED_KEY:
//           max(r, g, b) >= threshold on the stored bytes, no depth read.  DIST_INVERT takes the complement.  Pixels
//           outside the frame are never seeds.
//   field : d2(x, y) = min over seeds (sx, sy) of (x - sx)^2 + (y - sy)^2 where that is <= R^2, else DIST_FAR (0xFFFF);
//           R^2 <= 65025 < 0xFFFF.  A tap more than R away in either axis cannot give a value <= R^2, so the capped field
//           is exactly the minimum over |dx| <= R, |dy| <= R: two local passes, nothing approximated.
//   passes: a MASK of one bit a pixel (64-bit words, rows top down like the frame buffer, bits past the width 0); a ROW
//           pass h(x, y) = min(255, horizontal distance to the nearest set bit of the row), a byte, straight from the
//           words by count-leading / count-trailing zeros; a COLUMN pass d2 = min over |dy| <= R of dy^2 + h(x, y + dy)^2,
//           searched outwards dy = 0, 1, 2, .. with the exact exit dy^2 >= best.  The byte 255 means "255 or more": a tap
//           with dy >= 1 and h = 255 exceeds 65025 and counts as infinite; the pixel's OWN row (dy = 0) at R = 255 is
//           asked of the mask again, where 255 exactly and "none" differ (dist_own_row).
//   ramp  : dq = floor(sqrt(d2 * 65536)) (dist_isqrt, integers only), p = (dq * step) >> 8 with step = 1..65536 table
//           positions (1/256 of an entry) per pixel of distance; then the depth ramp's rule by its own functions
//           (tr_ramp.h): clamp to pmax or % pmax, ramp_entry, coverage e_a * opacity, tr_layer.h's layer_px.  A FAR pixel
//           takes the parameters' `far` entry; with DIST_KEEP_SEEDS a seed (d2 == 0) has coverage 0.
// One text for the device and the host compiler.
#pragma once

#include <stdint.h>

#include <vector>

#include "tr_layer.h"
#include "tr_math.h"
#include "tr_ramp.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t DIST_SEED_DRAWN = 0u, DIST_SEED_KEY = 1u;  // (= TR_DIST_SEED_*)
constexpr uint32_t DIST_INVERT = 0x1u;                        // (= TR_DIST_INVERT) tr_distance_params.flags
constexpr uint32_t DIST_REPEAT = 0x1u, DIST_KEEP_SEEDS = 0x2u;  // (= TR_DIST_REPEAT, TR_DIST_KEEP_SEEDS) tr_distance_ramp_params.flags
constexpr uint32_t DIST_MAX_RADIUS = 255u, DIST_FAR = 0xFFFFu, DIST_MAX_STEP = 65536u;
constexpr uint32_t DIST_NONE = 256u;        // a row distance: no set bit within 255
constexpr uint32_t DIST_INF = 0x7FFFFFFFu;  // a squared distance: no candidate yet

static_assert(DIST_MAX_RADIUS * DIST_MAX_RADIUS < DIST_FAR, "a kept squared distance is never DIST_FAR");
static_assert((uint64_t)DIST_MAX_RADIUS * DIST_MAX_RADIUS * 65536u < (1ull << 32), "d2 << 16 fits a u32");
static_assert((uint64_t)DIST_MAX_RADIUS * 256u * DIST_MAX_STEP < (1ull << 32), "dq * step fits a u32");

// The numbers of a field call, and of a ramp call with the table's length beside them.
struct DistRule {
    uint32_t seed, threshold, radius, flags;
};
struct DistRampRule {
    DistRule field;
    uint32_t step, mode, opacity, far, flags, n;
};

TR_HD uint32_t dist_words_per_row(uint32_t width) { return (width + 63u) / 64u; }

// Is the pixel (packed colour px, depth z; z is not looked at under DIST_SEED_KEY) a seed, before DIST_INVERT?
TR_HD bool dist_seed_key(uint32_t px, uint32_t threshold)
{
    const uint32_t r = px & 0xFFu, g = (px >> 8) & 0xFFu, b = (px >> 16) & 0xFFu;
    const uint32_t m = r > g ? (r > b ? r : b) : (g > b ? g : b);
    return m >= threshold;
}
TR_HD bool dist_seed_drawn(float z) { return layer_drawn(z); }

// Leading / trailing zeros of a word that is not 0.
TR_HD uint32_t dist_clz(uint64_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__clzll((long long)m);
#else
    return (uint32_t)__builtin_clzll(m);
#endif
}
TR_HD uint32_t dist_ctz(uint64_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(__ffsll((unsigned long long)m) - 1);
#else
    return (uint32_t)__builtin_ctzll(m);
#endif
}

// The horizontal distance from pixel x to the nearest set bit of its row (`row`: the row's wpr mask words), 0..255, or
// DIST_NONE.  At most four words beyond the pixel's own on either side: the fifth starts more than 255 away.
TR_HD uint32_t dist_row_exact(const uint64_t *row, uint32_t wpr, uint32_t x)
{
    const uint32_t w = x >> 6, b = x & 63u;
    uint32_t left = DIST_NONE, right = DIST_NONE;
    uint64_t m = row[w] & (~0ull >> (63u - b));  // the bits at and below b
    if (m != 0ull) {
        left = b - (63u - dist_clz(m));
    } else {
        uint32_t base = b + 1u;  // the distance to bit 63 of the word before
        for (uint32_t k = 1u; k <= 4u && k <= w; k++, base += 64u) {
            m = row[w - k];
            if (m != 0ull) {
                left = base + dist_clz(m);
                break;
            }
        }
    }
    m = row[w] >> b;  // bit 0: the pixel itself
    if (m != 0ull) {
        right = dist_ctz(m);
    } else {
        uint32_t base = 64u - b;  // the distance to bit 0 of the word after
        for (uint32_t k = 1u; k <= 4u && w + k < wpr; k++, base += 64u) {
            m = row[w + k];
            if (m != 0ull) {
                right = base + dist_ctz(m);
                break;
            }
        }
    }
    const uint32_t d = left < right ? left : right;
    return d < DIST_NONE ? d : DIST_NONE;
}

// The row pass's byte of a row distance: 255 stands for "255 or more".
TR_HD uint32_t dist_row_byte(uint32_t d) { return d < 255u ? d : 255u; }

// The summary byte of a row distance, the least of which over 64 pixels of a row says whether a column search through
// that row can find anything: never more than the distance, 255 only for DIST_NONE (254 stands for 254 and 255).  A
// search with radius R may skip the row where dist_summary_reach says so.
TR_HD uint32_t dist_summary_byte(uint32_t d) { return d == DIST_NONE ? 255u : (d < 254u ? d : 254u); }

// May a search with radius R find anything in a row whose summary byte is b?  (255 is "none" at every radius.)
TR_HD bool dist_summary_reach(uint32_t b, uint32_t R) { return b <= (R < 254u ? R : 254u); }

// The pixel's own row distance for the column pass from its byte h0: the byte itself, but for 255 at R = 255, where the
// mask says whether it is 255 exactly.
TR_HD uint32_t dist_own_row(uint32_t h0, uint32_t R, const uint64_t *row, uint32_t wpr, uint32_t x)
{
    if (h0 < 255u) return h0;
    if (R < 255u) return DIST_NONE;
    return dist_row_exact(row, wpr, x);
}

// The column pass of pixel (x, r): h is the byte plane (row stride `stride`, rows top down), own the pixel's own row
// distance (dist_own_row), H the number of rows.  Returns d2 or DIST_FAR; *taps (may be null) counts the bytes read.
TR_HD uint32_t dist_column(const uint8_t *h, size_t stride, uint32_t x, uint32_t r, uint32_t H, uint32_t R, uint32_t own, uint32_t *taps)
{
    uint32_t best = own <= R ? own * own : DIST_INF;
    uint32_t n = 0u;
    for (uint32_t dy = 1u; dy <= R && dy * dy < best; dy++) {
        const uint32_t dy2 = dy * dy;
        if (r >= dy) {
            const uint32_t v = h[(size_t)(r - dy) * stride + x];
            n++;
            if (v < 255u) {
                const uint32_t c = dy2 + v * v;
                best = c < best ? c : best;
            }
        }
        if (r + dy < H) {
            const uint32_t v = h[(size_t)(r + dy) * stride + x];
            n++;
            if (v < 255u) {
                const uint32_t c = dy2 + v * v;
                best = c < best ? c : best;
            }
        }
    }
    if (taps) *taps = n;
    return best <= R * R ? best : DIST_FAR;
}

// floor(sqrt(v)) of any u32, digit by digit in integers: r collects the root's bits from the top, v the remainder.
TR_HD uint32_t dist_isqrt(uint32_t v)
{
    uint32_t r = 0u;
    for (uint32_t bit = 1u << 30; bit != 0u; bit >>= 2) {
        const uint32_t t = r + bit;
        r >>= 1;
        if (v >= t) v -= t, r += bit;
    }
    return r;
}

// dq of a kept d2 (<= 65025): the distance in 1/256 of a pixel, <= 65280.
TR_HD uint32_t dist_dq(uint32_t d2) { return dist_isqrt(d2 << 16); }

// The table position of a kept d2, in 1/256 of a table step, before the clamp or the wrap.
TR_HD uint32_t dist_position_raw(uint32_t d2, uint32_t step) { return (dist_dq(d2) * step) >> 8; }

// ... and after it: 0 .. (n - 1) * 256.
TR_HD uint32_t dist_position(uint32_t d2, const DistRampRule &q)
{
    const uint32_t p = dist_position_raw(d2, q.step);
    const uint32_t pmax = (q.n - 1u) << 8;
    if (q.flags & DIST_REPEAT) return p % pmax;
    return p < pmax ? p : pmax;
}

// What a pixel with field value d2 blends: the interpolated entry, or `far`.
TR_HD uint32_t dist_source(const uint32_t *table, uint32_t d2, const DistRampRule &q)
{
    const uint32_t kept = d2 == DIST_FAR ? 0u : d2;  // (a FAR pixel computes a position like any other: no divergence)
    const uint32_t e = ramp_entry(table, q.n, dist_position(kept, q));
    return d2 == DIST_FAR ? q.far : e;
}

// The coverage of the source e over a pixel with field value d2.
TR_HD uint32_t dist_coverage(uint32_t e, uint32_t d2, const DistRampRule &q)
{
    if ((q.flags & DIST_KEEP_SEEDS) && d2 == 0u) return 0u;
    return ramp_coverage(e, q.opacity);
}

// The mask of a frame on the host: wpr words a row, rows top down.  z (index x + y * W, y up) may be null under KEY.
inline void distance_mask_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const DistRule &q, uint64_t *mask)
{
    const size_t W = width, H = height, wpr = dist_words_per_row(width);
    const bool invert = (q.flags & DIST_INVERT) != 0u;
    for (size_t r = 0; r < H; r++)
        for (size_t w = 0; w < wpr; w++) {
            uint64_t word = 0ull;
            for (size_t b = 0; b < 64u && w * 64u + b < W; b++) {
                const size_t x = w * 64u + b;
                const uint8_t *c = rgb + (r * W + x) * 3;
                const bool seed = q.seed == DIST_SEED_KEY ? dist_seed_key((uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16), q.threshold)
                                                          : dist_seed_drawn(z[x + (H - 1 - r) * W]);
                if (seed != invert) word |= 1ull << b;
            }
            mask[r * wpr + w] = word;
        }
}

// The rule over a whole frame on the host (the body of tr_distance_host; the caller has checked the parameters): the
// three passes as the kernels run them.  out: W x H u16, row 0 = top.
inline void distance_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const DistRule &q, uint16_t *out)
{
    const size_t W = width, H = height, wpr = dist_words_per_row(width);
    std::vector<uint64_t> mask(H * wpr);
    std::vector<uint8_t> h(W * H);
    distance_mask_host(width, height, rgb, z, q, mask.data());
    for (size_t r = 0; r < H; r++)
        for (size_t x = 0; x < W; x++) h[r * W + x] = (uint8_t)dist_row_byte(dist_row_exact(mask.data() + r * wpr, (uint32_t)wpr, (uint32_t)x));
    for (size_t r = 0; r < H; r++)
        for (size_t x = 0; x < W; x++) {
            const uint32_t own = dist_own_row(h[r * W + x], q.radius, mask.data() + r * wpr, (uint32_t)wpr, (uint32_t)x);
            out[r * W + x] = (uint16_t)dist_column(h.data(), W, (uint32_t)x, (uint32_t)r, height, q.radius, own, nullptr);
        }
}

// The ramp over a whole frame on the host (the body of tr_distance_ramp_host).  The field is complete before a colour
// changes, so out may be rgb.
inline void distance_ramp_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const DistRampRule &q, const uint8_t *table,
                               uint8_t *out)
{
    const size_t npx = (size_t)width * height;
    std::vector<uint16_t> field(npx);
    distance_host(width, height, rgb, z, q.field, field.data());
    std::vector<uint32_t> words(q.n);
    ramp_expand(q.n, table, words.data());
    for (size_t i = 0; i < npx; i++) {
        const uint8_t *sp = rgb + i * 3;
        uint8_t *o = out + i * 3;
        const uint32_t d = (uint32_t)sp[0] | ((uint32_t)sp[1] << 8) | ((uint32_t)sp[2] << 16);
        const uint32_t e = dist_source(words.data(), field[i], q);
        const uint32_t v = layer_px_by(q.mode, e, d, dist_coverage(e, field[i], q));
        o[0] = (uint8_t)(v & 0xFFu), o[1] = (uint8_t)((v >> 8) & 0xFFu), o[2] = (uint8_t)((v >> 16) & 0xFFu);
    }
}

// The arguments of k_dist_mask, k_dist_row and k_dist, passed by value.  fb: rgb8, buffer row height - 1 - y; fbclean /
// zclean: the frame's per-tile fast-clear flags over its 128 x 16 tile grid (fbclean may be null; zclean is read under
// DIST_SEED_DRAWN only); z: the frame's depth, y up.  mask: height * wpr words; h: width * height bytes; summary:
// height * wpr bytes; field: width * height u16 at any 2-byte-aligned address.  All rows top down.
struct DistArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    const float *z;
    const uint32_t *zclean;
    uint64_t *mask;
    uint8_t *h;
    uint8_t *summary;
    uint16_t *field;
    DevFrame frame;
    DistRule rule;
};

// k_dist_apply's arguments, passed by value: RampArgs with the field in the place of the depth.  field: width * height
// u16, 8-byte aligned, complete before the kernel starts.
struct DistApplyArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *lower;
    const uint16_t *field;
    const uint32_t *table;
    DevFrame frame;
    DistRampRule rule;
};

}  // namespace tr
