// tr_bilateral.h -- the rule of the bilateral stage (k_bilateral, tr_bilateral_host): a finished colour frame through an
// edge-preserving weighted mean whose weights fall with a tap's difference from the centre, in colour or in depth.  F is
// the frame as tr_scene_get_frame_buffer returns it: rgb8, row 0 = top, y grows downward; z is the depth as tr_dof_host
// takes it: index x + y * W, y UP, a pixel is not drawn when bits(z) == bits(f32::MIN).
//   window   : kw x kh, each odd and 1..15; spatial[j * kw + i] is the u8 weight of column i from the left, row j from
//              the TOP; a weight of 0 is no tap.  Tap (i, j) of pixel (x, y) reads position (x + i - kw / 2, y + j - kh / 2)
//   edge     : a tap outside the image has colour border[c] and depth f32::MIN under BORDER; under CLAMP its index is
//              clamped per axis, for colour and depth alike
//   distance : d of a tap T from the centre C, 0..255.  COLOUR: max(|Tr - Cr|, |Tg - Cg|, |Tb - Cb|).  DEPTH:
//              t = fl(|fl(zT - zC)| * depth_scale), every f32 operation rounded once, d = t < 255.0f ? (u32)t : 255 -- a
//              NaN or an infinity gives 255, two undrawn pixels give 0
//   weight   : w = spatial * range[d] <= 65025;  S = sum w;  A_c = sum w * T_c;  out_c = S == 0 ? C_c : (A_c + S / 2) / S
// Bounds: S <= 225 * 65025 = 14,630,625 < 2^24; A_c + S / 2 <= 225 * 65025 * 255 + 7,315,312 = 3,738,124,687 < 2^32: u32
// accumulators suffice and each product fits a 24-bit multiply (both factors below 2^24, the result below 2^32).  All
// integers: the order of the taps does not matter, and a window of zeros gives 0 (S == 0 gives the centre, which is 0
// too).  One text for the device and the host compiler.
#pragma once

#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t BILATERAL_GUIDE_COLOUR = 0u, BILATERAL_GUIDE_DEPTH = 1u;  // (= TR_BILATERAL_GUIDE_*)
constexpr uint32_t BILATERAL_BORDER = 0u, BILATERAL_CLAMP = 1u;
constexpr uint32_t BILATERAL_MAX_SIDE = 15u, BILATERAL_MAX_TAPS = BILATERAL_MAX_SIDE * BILATERAL_MAX_SIDE;
static_assert((uint64_t)BILATERAL_MAX_TAPS * 65025u < (1u << 24), "S fits 24 bits");
static_assert((uint64_t)BILATERAL_MAX_TAPS * 65025u * 255u + (uint64_t)BILATERAL_MAX_TAPS * 65025u / 2u < (1ull << 32), "A_c + S / 2 fits 32 bits");

// tr_bilateral_params, field for field (tr_scene.cpp asserts the two layouts equal).
struct BilateralParams {
    uint32_t struct_size, kw, kh, guide, edge;
    float depth_scale;
    uint8_t border[3];
    uint8_t pad;
    uint8_t spatial[BILATERAL_MAX_TAPS];
    uint8_t pad2[3];
    uint8_t range[256];
};
static_assert(sizeof(BilateralParams) == 512, "tr_bilateral_params is 512 bytes");

// The numbers of a call, as the kernel takes them by value: the byte tables as little-endian words.
struct BilateralRule {
    uint32_t kw, kh, guide, edge;
    uint32_t border;  // r | g << 8 | b << 16
    float depth_scale;
    uint32_t spatial[(BILATERAL_MAX_TAPS + 3u) / 4u];  // byte j * kw + i
    uint32_t range[64];                                // byte d
};

// Why the parameters are refused -- the text behind the entry point's name --, or null.
inline const char *bilateral_refusal(const BilateralParams &p)
{
    if (p.struct_size != sizeof(BilateralParams)) return ": struct_size is not sizeof(tr_bilateral_params)";
    if (p.kw % 2u == 0u || p.kh % 2u == 0u || p.kw > BILATERAL_MAX_SIDE || p.kh > BILATERAL_MAX_SIDE) return ": kw and kh must be odd and 1..15";
    bool any = false;
    for (uint32_t k = 0; k < BILATERAL_MAX_TAPS; k++) {
        if (k >= p.kw * p.kh && p.spatial[k] != 0u) return ": spatial weights outside the kw x kh window";
        any = any || p.spatial[k] != 0u;
    }
    if (!any) return ": the window is all zeros";
    if (p.guide != BILATERAL_GUIDE_COLOUR && p.guide != BILATERAL_GUIDE_DEPTH) return ": guide must be TR_BILATERAL_GUIDE_COLOUR or TR_BILATERAL_GUIDE_DEPTH";
    if (p.edge != BILATERAL_BORDER && p.edge != BILATERAL_CLAMP) return ": edge must be TR_BILATERAL_BORDER or TR_BILATERAL_CLAMP";
    if (!(p.depth_scale >= 0.0f) || !(p.depth_scale <= 3.402823466e38f)) return ": depth_scale must be finite and >= 0";
    if (p.pad != 0u || p.pad2[0] != 0u || p.pad2[1] != 0u || p.pad2[2] != 0u) return ": pad and pad2 must be 0";
    return nullptr;
}

// (of parameters that are not refused)
inline BilateralRule bilateral_rule(const BilateralParams &p)
{
    BilateralRule r = {};
    r.kw = p.kw, r.kh = p.kh, r.guide = p.guide, r.edge = p.edge, r.depth_scale = p.depth_scale;
    r.border = (uint32_t)p.border[0] | ((uint32_t)p.border[1] << 8) | ((uint32_t)p.border[2] << 16);
    for (uint32_t k = 0; k < p.kw * p.kh; k++) r.spatial[k / 4u] |= (uint32_t)p.spatial[k] << (8u * (k % 4u));
    for (uint32_t d = 0; d < 256u; d++) r.range[d / 4u] |= (uint32_t)p.range[d] << (8u * (d % 4u));
    return r;
}

// Byte k of a table of little-endian words.
TR_HD uint32_t bilateral_byte(const uint32_t *words, uint32_t k) { return (words[k / 4u] >> (8u * (k % 4u))) & 0xFFu; }

TR_HD uint32_t bilateral_absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

// COLOUR: the distance of the packed pixels (r | g << 8 | b << 16) t and c.
TR_HD uint32_t bilateral_colour_distance(uint32_t t, uint32_t c)
{
    const uint32_t dr = bilateral_absdiff(t & 0xFFu, c & 0xFFu), dg = bilateral_absdiff((t >> 8) & 0xFFu, (c >> 8) & 0xFFu), db = bilateral_absdiff(t >> 16, c >> 16);
    const uint32_t m = dr > dg ? dr : dg;
    return m > db ? m : db;
}

// DEPTH: the distance of the depths zt and zc.  Two roundings (the build has no contraction, and there is nothing to
// contract: a difference, an absolute value, a product); the comparison is false for a NaN, and an infinity is not below 255.
TR_HD uint32_t bilateral_depth_distance(float zt, float zc, float depth_scale)
{
    const float diff = zt - zc;
    const float t = (diff < 0.0f ? -diff : diff) * depth_scale;
    return t < 255.0f ? (uint32_t)t : 255u;
}

// The sums of one pixel and their finish: S and A_c in u32 (the bounds above).
struct BilateralSums {
    uint32_t s, a[3];
};

// One tap of weight w = spatial * range[d] on the packed pixel t.  (Both factors of every product are below 2^24: mul24.)
TR_HD void bilateral_tap(BilateralSums &m, uint32_t w, uint32_t t)
{
    m.s += w;
    m.a[0] += mul24(w, t & 0xFFu);
    m.a[1] += mul24(w, (t >> 8) & 0xFFu);
    m.a[2] += mul24(w, t >> 16);
}

// The finished packed pixel from the sums and the centre c.
TR_HD uint32_t bilateral_finish_px(const BilateralSums &m, uint32_t c)
{
    if (m.s == 0u) return c;
    const uint32_t h = m.s / 2u;
    return (m.a[0] + h) / m.s | ((m.a[1] + h) / m.s << 8) | ((m.a[2] + h) / m.s << 16);
}

// The rule over a whole frame on the host (the body of tr_bilateral_host; the caller has checked the parameters).  rgb
// and out: row 0 = top, out != rgb; z: x + y * W, y up, read only under the DEPTH guide (may be null otherwise).
inline void bilateral_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, uint8_t *out, const BilateralRule &q)
{
    const int64_t W = width, H = height, kw = q.kw, kh = q.kh, rx = kw / 2, ry = kh / 2;
    const bool clamp = q.edge == BILATERAL_CLAMP, depth = q.guide == BILATERAL_GUIDE_DEPTH;
    const float z_min = bits_f32(TR_F32_MIN_BITS);
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            const uint8_t *f = rgb + (y * W + x) * 3;
            const uint32_t c = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16);
            const float zc = depth ? z[(H - 1 - y) * W + x] : 0.0f;
            BilateralSums m = { 0u, { 0u, 0u, 0u } };
            for (int64_t j = 0; j < kh; j++) {
                int64_t yy = y + j - ry;
                const bool y_out = yy < 0 || yy >= H;
                yy = yy < 0 ? 0 : yy >= H ? H - 1 : yy;
                for (int64_t i = 0; i < kw; i++) {
                    const uint32_t sw = bilateral_byte(q.spatial, (uint32_t)(j * kw + i));
                    if (sw == 0u) continue;
                    int64_t xx = x + i - rx;
                    const bool outside = y_out || xx < 0 || xx >= W;
                    xx = xx < 0 ? 0 : xx >= W ? W - 1 : xx;
                    uint32_t t = q.border;
                    float zt = z_min;
                    if (clamp || !outside) {
                        const uint8_t *g = rgb + (yy * W + xx) * 3;
                        t = (uint32_t)g[0] | ((uint32_t)g[1] << 8) | ((uint32_t)g[2] << 16);
                        if (depth) zt = z[(H - 1 - yy) * W + xx];
                    }
                    const uint32_t d = depth ? bilateral_depth_distance(zt, zc, q.depth_scale) : bilateral_colour_distance(t, c);
                    bilateral_tap(m, mul24(sw, bilateral_byte(q.range, d)), t);
                }
            }
            const uint32_t v = bilateral_finish_px(m, c);
            uint8_t *o = out + (y * W + x) * 3;
            o[0] = (uint8_t)(v & 0xFFu), o[1] = (uint8_t)((v >> 8) & 0xFFu), o[2] = (uint8_t)(v >> 16);
        }
}

// k_bilateral's arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y for the kernel's row y (row 0 =
// bottom), out does not overlap fb; z: index x + y * width, y up, read only under the DEPTH guide; fbclean / zclean: the
// scene's per-tile fast-clear flags over the whole frame's tile grid (band scenes are refused; either may be null: nothing
// is known); out_clean: null, or where the workgroup writes the flag of its tile of `out`.  words: fb is 4-byte aligned
// and the width a multiple of 4, so four pixels at a multiple of four are three aligned words.
struct BilateralArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    const float *z;
    const uint32_t *zclean;
    uint8_t *out;
    uint32_t *out_clean;
    DevFrame frame;
    uint32_t words;
    BilateralRule rule;
};

}  // namespace tr
