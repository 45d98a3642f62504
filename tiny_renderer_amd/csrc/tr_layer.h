// tr_layer.h -- the rule of layers (k_layer, tr_layer_host): a second image L -- w x h pixels, rgb8 or rgba8, rows
// `stride` bytes apart -- is blended into a finished colour frame F with its top-left pixel on frame pixel (x, y), x and
// y signed: the layer may hang over any edge or miss the frame.  F is W x H, row 0 = top, as stored.  For a frame pixel
// P inside the layer's rectangle, s is the layer's pixel there and d the frame's; per channel:
//   coverage : a = A * opacity, A the layer's alpha byte (255 for rgb8), opacity 0..256: a in 0..65280.  With LAYER_KEY a
//              layer pixel whose rgb equals `key` has a = 0; with LAYER_WHERE_DRAWN a = 0 where the frame's own depth at P
//              says nothing is drawn (bits(z) == bits(f32::MIN)); with LAYER_WHERE_UNDRAWN a = 0 where something is.
//   blend    : b = s (NORMAL), min(255, s + d) (ADD), (s d + 127) / 255 (MULTIPLY), 255 - ((255 - s)(255 - d) + 127) / 255
//              (SCREEN), max(s, d) (LIGHTEN), min(s, d) (DARKEN), |s - d| (DIFFERENCE).
//   output   : (b a + d (65280 - a) + 32640) / 65280, rounded once.
// Both divisions are exact in 32-bit integers without a divide: n / 65280 = ((n >> 8) * 0x8081) >> 23 for n up to
// 255 * 65280 + 32640, and x / 255 = (x * 0x8081) >> 23 for x < 65536.  A frame pixel outside the rectangle is unchanged.
// It follows: opacity 0 or A = 0 leaves d; A = 255 at opacity 256 gives exactly b.  Only colour changes: z, winner words
// and the shadow buffer stay, so a backdrop pixel is still "not drawn" to a later composite, outline or depth of field.
// A pixel depends on itself and on the layer alone: the rule works in place.  z is indexed x + y * W, y up (tr_ao.h).
// One text for the device and the host compiler.
#pragma once

#include <stdint.h>
#include <string.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t LAYER_NORMAL = 0u, LAYER_ADD = 1u, LAYER_MULTIPLY = 2u, LAYER_SCREEN = 3u, LAYER_LIGHTEN = 4u, LAYER_DARKEN = 5u,
                   LAYER_DIFFERENCE = 6u, LAYER_MODES = 7u;                  // (= TR_LAYER_NORMAL ..)
constexpr uint32_t LAYER_RGB8 = 0u, LAYER_RGBA8 = 1u;                        // (= TR_LAYER_RGB8, TR_LAYER_RGBA8)
constexpr uint32_t LAYER_KEY = 0x1u, LAYER_WHERE_DRAWN = 0x2u, LAYER_WHERE_UNDRAWN = 0x4u;  // (= TR_LAYER_KEY ..)
constexpr uint32_t LAYER_MAX_SIDE = 8192u, LAYER_FULL = 65280u;

// The numbers of a call: the header's tr_layer_params with the stride made real (never 0) and the key as a packed pixel
// (r in bits 0..7, g in 8..15, b in 16..23).
struct LayerRule {
    uint32_t mode, format, flags, opacity;
    int32_t x, y;
    uint32_t width, height, stride, key;
};

TR_HD uint32_t layer_bpp(uint32_t format) { return format == LAYER_RGBA8 ? 4u : 3u; }

// The bytes from the layer's first to its last: what a call may read of `image`.
TR_HD int64_t layer_block_bytes(uint32_t width, uint32_t height, uint32_t stride, uint32_t format)
{
    return (int64_t)stride * (int64_t)(height - 1u) + (int64_t)width * (int64_t)layer_bpp(format);
}

// x / 255 for x < 65536.
TR_HD uint32_t layer_div255(uint32_t x) { return mul24(x, 0x8081u) >> 23; }

// n / 65280 for n <= 255 * 65280 + 32640.
TR_HD uint32_t layer_div65280(uint32_t n) { return mul24(n >> 8, 0x8081u) >> 23; }

// One channel of the blend.
template <uint32_t MODE>
TR_HD uint32_t layer_blend(uint32_t s, uint32_t d)
{
    if (MODE == LAYER_ADD) return s + d > 255u ? 255u : s + d;
    if (MODE == LAYER_MULTIPLY) return layer_div255(mul24(s, d) + 127u);
    if (MODE == LAYER_SCREEN) return 255u - layer_div255(mul24(255u - s, 255u - d) + 127u);
    if (MODE == LAYER_LIGHTEN) return s > d ? s : d;
    if (MODE == LAYER_DARKEN) return s < d ? s : d;
    if (MODE == LAYER_DIFFERENCE) return s > d ? s - d : d - s;
    return s;
}

// One channel of the output: the blend b over the frame's d under coverage a (0..65280).
TR_HD uint32_t layer_mix(uint32_t b, uint32_t d, uint32_t a) { return layer_div65280(mul24(b, a) + mul24(d, LAYER_FULL - a) + 32640u); }

// A whole pixel, packed: s the layer's (its bits 24..31 are not looked at), d the frame's, a the coverage.
template <uint32_t MODE>
TR_HD uint32_t layer_px(uint32_t s, uint32_t d, uint32_t a)
{
    uint32_t o = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; c++) {
        const uint32_t sc = (s >> (8 * c)) & 0xFFu, dc = (d >> (8 * c)) & 0xFFu;
        o |= layer_mix(layer_blend<MODE>(sc, dc), dc, a) << (8 * c);
    }
    return o;
}

// The same with the mode as a number.
TR_HD uint32_t layer_px_by(uint32_t mode, uint32_t s, uint32_t d, uint32_t a)
{
    switch (mode) {
    case LAYER_ADD: return layer_px<LAYER_ADD>(s, d, a);
    case LAYER_MULTIPLY: return layer_px<LAYER_MULTIPLY>(s, d, a);
    case LAYER_SCREEN: return layer_px<LAYER_SCREEN>(s, d, a);
    case LAYER_LIGHTEN: return layer_px<LAYER_LIGHTEN>(s, d, a);
    case LAYER_DARKEN: return layer_px<LAYER_DARKEN>(s, d, a);
    case LAYER_DIFFERENCE: return layer_px<LAYER_DIFFERENCE>(s, d, a);
    default: return layer_px<LAYER_NORMAL>(s, d, a);
    }
}

// The coverage of a layer pixel s (rgb in bits 0..23, alpha in 24..31: 255 for rgb8) on a frame pixel that is drawn or not.
TR_HD uint32_t layer_coverage(const LayerRule &q, uint32_t s, bool drawn)
{
    if ((q.flags & LAYER_KEY) && (s & 0xFFFFFFu) == q.key) return 0u;
    if ((q.flags & LAYER_WHERE_DRAWN) && !drawn) return 0u;
    if ((q.flags & LAYER_WHERE_UNDRAWN) && drawn) return 0u;
    return mul24(s >> 24, q.opacity);
}

TR_HD bool layer_drawn(float z) { return f32_bits(z) != TR_F32_MIN_BITS; }

// Bytes sh .. sh + 3 of the eight bytes (lo, hi), sh = 0..3.
TR_HD uint32_t layer_funnel(uint32_t lo, uint32_t hi, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return sh == 0u ? lo : (lo >> (8u * sh)) | (hi << (32u - 8u * sh));
#endif
}

// The four bytes at offset `at` of the block image[0 .. total), image + at a multiple of 4 as an address, for a reader
// that needs bytes [need0, need1) of the block (0 <= need0 <= need1 <= total) and nothing else.  A word that does not
// overlap them is NOT loaded (it may lie outside the caller's memory) and reads as 0; one that lies inside the block is
// one aligned load; the block's first or last word, where it reaches outside, is put together from its needed bytes.
TR_HD uint32_t layer_word(const uint8_t *image, int64_t total, int64_t at, int64_t need0, int64_t need1)
{
    if (at + 4 <= need0 || at >= need1) return 0u;
    if (at >= 0 && at + 4 <= total) return *reinterpret_cast<const uint32_t *>(image + at);
    uint32_t v = 0u;
    for (int k = 0; k < 4; k++)
        if (at + k >= need0 && at + k < need1) v |= (uint32_t)image[at + k] << (8 * k);
    return v;
}

// Four consecutive layer pixels of BPP bytes each, the first at byte offset u0 of the block (which may lie before the
// block or run past it: a unit the rectangle only partly covers), from the aligned words that cover them, funnel-shifted:
// px[i] = rgb in bits 0..23, alpha in 24..31 (255 for BPP = 3).  Only bytes [need0, need1) count: a pixel outside them
// comes out as whatever the words not loaded leave, and the caller does not look at it.
template <int BPP>
TR_HD void layer_fetch(const uint8_t *image, int64_t total, int64_t u0, int64_t need0, int64_t need1, uint32_t px[4])
{
    constexpr int NW = BPP == 3 ? 4 : 5;
    const uint32_t sh = (uint32_t)((uint64_t)(uintptr_t)image + (uint64_t)u0) & 3u;
    const int64_t at = u0 - (int64_t)sh;
    uint32_t w[NW], t[NW - 1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < NW; k++) w[k] = layer_word(image, total, at + 4 * k, need0, need1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < NW - 1; k++) t[k] = layer_funnel(w[k], w[k + 1], sh);
    if (BPP == 3) {
        px[0] = (t[0] & 0xFFFFFFu) | 0xFF000000u;
        px[1] = (t[0] >> 24) | ((t[1] & 0xFFFFu) << 8) | 0xFF000000u;
        px[2] = (t[1] >> 16) | ((t[2] & 0xFFu) << 16) | 0xFF000000u;
        px[3] = (t[2] >> 8) | 0xFF000000u;
    } else {
        px[0] = t[0], px[1] = t[1], px[2] = t[2], px[3] = t[NW - 2];
    }
}

// The rule over a whole frame on the host (the body of tr_layer_host; the caller has checked the parameters).  rgb and
// out: W x H rgb8, row 0 = top; out may be rgb; z (index x + y * W, y up) is only read with a WHERE flag.
inline void layer_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const LayerRule &q, const uint8_t *image, uint8_t *out)
{
    const int64_t W = width, H = height, bpp = layer_bpp(q.format);
    if (out != rgb) memmove(out, rgb, (size_t)(W * H * 3));
    const int64_t x0 = q.x < 0 ? 0 : q.x, y0 = q.y < 0 ? 0 : q.y;
    const int64_t x1 = (int64_t)q.x + q.width < W ? (int64_t)q.x + q.width : W, y1 = (int64_t)q.y + q.height < H ? (int64_t)q.y + q.height : H;
    for (int64_t r = y0; r < y1; r++)
        for (int64_t x = x0; x < x1; x++) {
            const uint8_t *sp = image + (r - q.y) * (int64_t)q.stride + (x - q.x) * bpp;
            const uint32_t s = (uint32_t)sp[0] | ((uint32_t)sp[1] << 8) | ((uint32_t)sp[2] << 16) | ((bpp == 4 ? (uint32_t)sp[3] : 255u) << 24);
            const bool drawn = (q.flags & (LAYER_WHERE_DRAWN | LAYER_WHERE_UNDRAWN)) ? layer_drawn(z[x + (H - 1 - r) * W]) : false;
            uint8_t *o = out + (r * W + x) * 3;
            const uint32_t d = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
            const uint32_t v = layer_px_by(q.mode, s, d, layer_coverage(q, s, drawn));
            o[0] = (uint8_t)(v & 0xFFu), o[1] = (uint8_t)((v >> 8) & 0xFFu), o[2] = (uint8_t)((v >> 16) & 0xFFu);
        }
}

// k_layer's arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y; out is fb (in place) or does not
// overlap it.  image: the layer's block of `total` bytes (layer_block_bytes), any alignment; it overlaps neither.
// z / zclean: only with a WHERE flag.  src_clean: null, or (the layer is another scene's frame) that frame's colour
// fast-clear flags over its 128 x 16 tile grid, src_ntx a row, counted from the frame's bottom row; src_all_clean: that
// frame is logically cleared, nothing of it is loaded.  c*: the layer's rectangle clipped to the frame, columns
// [cx0, cx1) and rows from the top [cr0, cr1), empty where it misses.  g*: the tiles launched, gnx x (grid / gnx) from
// tile (gx0, gy0).  lower: in place, where the kernel lowers the colour flag of a flagged tile it has written.
struct LayerArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *lower;
    const float *z;
    const uint32_t *zclean;
    const uint8_t *image;
    int64_t total;
    const uint32_t *src_clean;
    uint32_t src_ntx, src_all_clean;
    DevFrame frame;
    LayerRule rule;
    int32_t cx0, cx1, cr0, cr1;
    uint32_t gx0, gy0, gnx, gny;
};

}  // namespace tr
