// tr_convolve.h -- the rule of the convolve stage (k_convolve, tr_convolve_host): a finished colour frame filtered through
// a kernel of integer weights.  F is the frame as tr_scene_get_frame_buffer returns it: rgb8, row 0 = top, y grows
// downward.  kw x kh taps, both odd; w(i, j) is the weight of column i from the left, row j from the top:
//   general   : w(i, j) = weights[j * kw + i], kw and kh 1..9
//   separable : row = weights[0 .. kw), col = weights[kw .. kw + kh), w(i, j) = row[i] * col[j], kw and kh 1..31
//   sum   : acc[c] = sum over j < kh, i < kw of w(i, j) * F(x + i - kw / 2, y + j - kh / 2)[c]      (correlation: no flip)
//           a tap outside the image is border[c] under BORDER; under CLAMP its index is clamped per axis
//   scale : v = (acc + rnd) >> shift, an arithmetic shift, rnd = shift ? 1 << (shift - 1) : 0;  under ABS v = |v|
//   out   : clamp(v + bias, 0, 255)
//           UNSHARP: v = clamp(v, 0, 255), out = clamp(F + ((amount * (F - v) + 128) >> 8), 0, 255), arithmetic shift
// Bounds.  A = sum |w| (general) or sum |row| * sum |col| (separable) is at most 2^22: |acc| + rnd <= 255 A + 2^21 < 2^31,
// so an int32 holds every sum, whole or partial, in any order.  Separable: sum |row| <= 2^15 as well, so a horizontal
// sum is below 255 * 2^15 < 2^23 and a vertical pass over horizontal sums may multiply in 24 bits.  The separable form
// is DEFINED as the 2-D sum of the outer product; everything is integer, so one pass after the other -- in either order
// -- gives the same bytes.  One text for the device and the host compiler.
#pragma once

#include <stdint.h>

#include <vector>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t CONVOLVE_SEPARABLE = 1u, CONVOLVE_ABS = 2u, CONVOLVE_UNSHARP = 4u;  // (= TR_CONVOLVE_*)
constexpr uint32_t CONVOLVE_BORDER = 0u, CONVOLVE_CLAMP = 1u;
constexpr int CONVOLVE_MAX_GENERAL = 9, CONVOLVE_MAX_SEPARABLE = 31, CONVOLVE_MAX_WEIGHTS = 82;
constexpr uint32_t CONVOLVE_MAX_SHIFT = 22u, CONVOLVE_MAX_AMOUNT = 1024u;
constexpr int32_t CONVOLVE_MAX_BIAS = 255;
constexpr int64_t CONVOLVE_MAX_A = 1ll << 22, CONVOLVE_MAX_ROW = 1ll << 15;

static_assert(255ll * CONVOLVE_MAX_A + (1ll << (CONVOLVE_MAX_SHIFT - 1)) < (1ll << 31), "an int32 holds every sum and its rounding term");
static_assert(81ll * 32767ll <= CONVOLVE_MAX_A && CONVOLVE_MAX_GENERAL * CONVOLVE_MAX_GENERAL + 1 == CONVOLVE_MAX_WEIGHTS,
              "no int16 kernel of the general form is refused on A");
static_assert(2 * CONVOLVE_MAX_SEPARABLE <= CONVOLVE_MAX_WEIGHTS, "a row and a column fit the weights");
static_assert(255ll * CONVOLVE_MAX_ROW < (1ll << 23), "a horizontal sum is a signed 24-bit factor");
static_assert((int64_t)CONVOLVE_MAX_AMOUNT * 255ll + 128ll < (1ll << 23) && 255ll * CONVOLVE_MAX_A + (1ll << 21) + CONVOLVE_MAX_BIAS < (1ll << 31),
              "the output step stays in an int32, amount * (F - v) in 24 bits");

// The numbers of a call, as the kernel takes them by value.
struct ConvolveRule {
    uint32_t kw, kh, flags, shift;
    int32_t bias;
    uint32_t amount, edge;
    uint32_t border;  // r | g << 8 | b << 16
    int32_t mul24;    // separable: sum |col| <= 2^15 as well, so a vertical sum is a signed 24-bit factor too
    int32_t weights[CONVOLVE_MAX_WEIGHTS];
};

// a * b where both are signed 24-bit numbers and the product fits an int32 (one full-rate instruction on the device).
TR_HD int32_t convolve_mul24(int32_t a, int32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

TR_HD int32_t convolve_clamp255(int32_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// scale and out: one channel from its sum `acc` and the frame's own value F.
TR_HD uint32_t convolve_finish(int32_t acc, int32_t F, const ConvolveRule &q)
{
    const int32_t rnd = q.shift != 0u ? (int32_t)(1u << (q.shift - 1u)) : 0;
    int32_t v = (acc + rnd) >> q.shift;
    if ((q.flags & CONVOLVE_ABS) != 0u && v < 0) v = -v;
    if ((q.flags & CONVOLVE_UNSHARP) != 0u) {
        v = convolve_clamp255(v);
        return (uint32_t)convolve_clamp255(F + ((convolve_mul24((int32_t)q.amount, F - v) + 128) >> 8));
    }
    return (uint32_t)convolve_clamp255(v + q.bias);
}

// The finished pixel, packed r | g << 8 | b << 16, from the three sums and the frame's packed pixel.
TR_HD uint32_t convolve_finish_px(int32_t r, int32_t g, int32_t b, uint32_t f, const ConvolveRule &q)
{
    return convolve_finish(r, (int32_t)(f & 0xFFu), q) | (convolve_finish(g, (int32_t)((f >> 8) & 0xFFu), q) << 8) |
           (convolve_finish(b, (int32_t)((f >> 16) & 0xFFu), q) << 16);
}

// What a neighbourhood of zeros becomes (every channel the same): clamp(bias), or 0 under UNSHARP.
TR_HD uint32_t convolve_of_zeros(const ConvolveRule &q) { return convolve_finish(0, 0, q); }

// w(i, j) of the general form; the row and the column of the separable one.
TR_HD int32_t convolve_weight(const ConvolveRule &q, uint32_t i, uint32_t j) { return q.weights[j * q.kw + i]; }
TR_HD int32_t convolve_row(const ConvolveRule &q, uint32_t i) { return q.weights[i]; }
TR_HD int32_t convolve_col(const ConvolveRule &q, uint32_t j) { return q.weights[q.kw + j]; }

// The rule over a whole frame on the host (the body of tr_convolve_host; the caller has checked the parameters).  rgb and
// out: row 0 = top, out != rgb.  Reads 3 * width * height bytes, writes as many.  The separable form runs a horizontal
// pass into int32 sums of the frame's size and a vertical pass over them; a row outside the image is the border's
// horizontal sum under BORDER and the clamped row's under CLAMP.
inline void convolve_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out, const ConvolveRule &q)
{
    const int64_t W = width, H = height, kw = q.kw, kh = q.kh, rx = kw / 2, ry = kh / 2;
    const bool clamp = q.edge == CONVOLVE_CLAMP;
    const int32_t border[3] = { (int32_t)(q.border & 0xFFu), (int32_t)((q.border >> 8) & 0xFFu), (int32_t)((q.border >> 16) & 0xFFu) };
    auto texel = [&](int64_t x, int64_t y, int c) -> int32_t {
        if (clamp) {
            x = x < 0 ? 0 : x >= W ? W - 1 : x;
            y = y < 0 ? 0 : y >= H ? H - 1 : y;
        } else if (x < 0 || x >= W || y < 0 || y >= H) {
            return border[c];
        }
        return rgb[(y * W + x) * 3 + c];
    };
    auto store = [&](int64_t x, int64_t y, const int32_t (&acc)[3]) {
        const uint8_t *f = rgb + (y * W + x) * 3;
        for (int c = 0; c < 3; c++) out[(y * W + x) * 3 + c] = (uint8_t)convolve_finish(acc[c], f[c], q);
    };
    if ((q.flags & CONVOLVE_SEPARABLE) == 0u) {
        for (int64_t y = 0; y < H; y++)
            for (int64_t x = 0; x < W; x++) {
                int32_t acc[3] = { 0, 0, 0 };
                for (int64_t j = 0; j < kh; j++)
                    for (int64_t i = 0; i < kw; i++) {
                        const int32_t w = convolve_weight(q, (uint32_t)i, (uint32_t)j);
                        if (w == 0) continue;
                        for (int c = 0; c < 3; c++) acc[c] += w * texel(x + i - rx, y + j - ry, c);
                    }
                store(x, y, acc);
            }
        return;
    }
    std::vector<int32_t> hs((size_t)(W * H * 3));
    int32_t hb[3] = { 0, 0, 0 };  // the horizontal sum of a row outside the image under BORDER
    for (int64_t i = 0; i < kw; i++)
        for (int c = 0; c < 3; c++) hb[c] += convolve_row(q, (uint32_t)i) * border[c];
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++)
            for (int c = 0; c < 3; c++) {
                int32_t h = 0;
                for (int64_t i = 0; i < kw; i++) h += convolve_row(q, (uint32_t)i) * texel(x + i - rx, y, c);
                hs[(size_t)((y * W + x) * 3 + c)] = h;
            }
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            int32_t acc[3] = { 0, 0, 0 };
            for (int64_t j = 0; j < kh; j++) {
                int64_t yy = y + j - ry;
                const bool outside = yy < 0 || yy >= H;
                if (clamp) yy = yy < 0 ? 0 : yy >= H ? H - 1 : yy;
                for (int c = 0; c < 3; c++)
                    acc[c] += convolve_col(q, (uint32_t)j) * (outside && !clamp ? hb[c] : hs[(size_t)((yy * W + x) * 3 + c)]);
            }
            store(x, y, acc);
        }
}

// k_convolve's arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y for the kernel's row y (row 0 =
// bottom), out does not overlap fb; fbclean: the scene's per-tile colour fast-clear flags over the whole frame's tile
// grid (band scenes are refused; may be null: nothing is known about the colour); out_clean: null, or where the
// workgroup writes the flag of its tile of `out`.  words: fb is 4-byte aligned and the width a multiple of 4, so four
// pixels at a multiple of four are three aligned words.
struct ConvolveArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *out_clean;
    DevFrame frame;
    uint32_t words;
    ConvolveRule rule;
};

}  // namespace tr
