// tr_yuv.h -- the rule of the YUV output stage (k_yuv, tr_yuv_host): a frame of W x H rgb8 converted to 8-bit YCbCr
// planes in the frame BUFFER's orientation (row 0 = top), tightly packed.  cw = (W + 1) / 2, ch = (H + 1) / 2.
//   YUV_I420 (0)  Y (W x H), U (cw x ch), V (cw x ch)                         W H + 2 cw ch bytes
//   YUV_NV12 (1)  Y (W x H), one plane of cw x ch interleaved (U, V) pairs    W H + 2 cw ch bytes
//   YUV_I444 (2)  Y, U, V, each W x H                                         3 W H bytes
// Coefficients are in units of 1 / 65536, rows (r, g, b): the nearest integers to the real matrix (for the limited range
// scaled by 219 / 255 for Y and 224 / 255 for chroma), the green entry adjusted so that a Y row sums to the rounded scale
// and a chroma row to exactly 0 (kYuvTables; tests/yuv_cases.py derives them again from Kr and Kb).  In i32 with
// arithmetic shifts:
//   Y = (yr R + yg G + yb B + (y0 << 16) + 32768) >> 16                       per pixel, every layout
//   U = (ur R + ug G + ub B + (128 << 16) + 32768) >> 16                      I444, per pixel; V with the V row
//   U = (ur Rs + ug Gs + ub Bs + (128 << 18) + (1 << 17)) >> 18               4:2:0; V with the V row
// where chroma sample (i, j) of 4:2:0 covers columns 2i and min(2i + 1, W - 1) and rows 2j and min(2j + 1, H - 1) -- at
// an odd edge the last column or row counts twice -- and Rs, Gs, Bs are the sums of those four pixels (0..1020), rounded
// once: the centred siting (C420jpeg).  Every result is clamped to 0..255; the clamp only ever acts at the top (full
// range: pure blue gives U = 256, pure red V = 256) and nothing goes negative.  The largest accumulator is
// 32768 * 1020 + (128 << 18) + (1 << 17) < 2^27.  A grey v gives Y = v in full range and U = V = 128 everywhere; black
// gives (y0, 128, 128) -- what a tile behind a raised colour flag becomes without a load.  This Y is NOT k_stats' 8-bit
// luma (54, 183, 19).  One text for the device and the host compiler.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t YUV_I420 = 0u, YUV_NV12 = 1u, YUV_I444 = 2u;  // (= TR_YUV_I420, TR_YUV_NV12, TR_YUV_I444)
constexpr uint32_t YUV_BT601 = 0u, YUV_BT709 = 1u;               // (= TR_YUV_BT601, TR_YUV_BT709)
constexpr uint32_t YUV_FULL = 0u, YUV_LIMITED = 1u;              // (= TR_YUV_FULL, TR_YUV_LIMITED)
constexpr uint32_t YUV_MAX_SIDE = 8192u;

// The numbers of a call: the three rows, Y's offset and the layout.
struct YuvRule {
    int32_t y[3], u[3], v[3];
    int32_t y0;
    uint32_t layout;
};

// [matrix][range]
constexpr YuvRule kYuvTables[2][2] = {
    { { { 19595, 38470, 7471 }, { -11058, -21710, 32768 }, { 32768, -27439, -5329 }, 0, 0u },
      { { 16829, 33039, 6416 }, { -9714, -19070, 28784 }, { 28784, -24103, -4681 }, 16, 0u } },
    { { { 13933, 46871, 4732 }, { -7509, -25259, 32768 }, { 32768, -29763, -3005 }, 0, 0u },
      { { 11966, 40254, 4064 }, { -6596, -22188, 28784 }, { 28784, -26145, -2639 }, 16, 0u } },
};

static_assert(32768 * 1020 + (128 << 18) + (1 << 17) < (1 << 27), "every accumulator stays below 2^27");

// The clamp.  On the device the result passes through an empty asm statement, which emits no instruction and only keeps
// the compiler from fusing "shift, clamp, pack two bytes" of neighbouring pixels into gfx950's v_ashr_pk_u8_i32: that
// instruction writes the low 16 bits of its destination and leaves the high 16 as they were, while the `or` the compiler
// puts behind it takes them for zeros -- bytes 2 and 3 of a packed word of Y came out as whatever the register held
// (seen on an MI355X with ROCm's hipcc at -O3; the byte form, which packs nothing, was right).
TR_HD uint32_t yuv_clamp(int32_t v)
{
    uint32_t r = (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
#if defined(__HIP_DEVICE_COMPILE__)
    asm("" : "+v"(r));
#endif
    return r;
}

// One row of the matrix over one pixel (r, g, b: 0..255) or one 4:2:0 block's sums (0..1020), before offset and shift.
TR_HD int32_t yuv_dot(const int32_t row[3], int32_t r, int32_t g, int32_t b) { return row[0] * r + row[1] * g + row[2] * b; }

// Y of one pixel.
TR_HD uint32_t yuv_luma(const YuvRule &k, int32_t r, int32_t g, int32_t b)
{
    return yuv_clamp((yuv_dot(k.y, r, g, b) + (k.y0 << 16) + 32768) >> 16);
}

// U or V of one pixel (I444).
TR_HD uint32_t yuv_chroma1(const int32_t row[3], int32_t r, int32_t g, int32_t b)
{
    return yuv_clamp((yuv_dot(row, r, g, b) + (128 << 16) + 32768) >> 16);
}

// U or V of one 4:2:0 sample from the sums of its four pixels.
TR_HD uint32_t yuv_chroma4(const int32_t row[3], int32_t rs, int32_t gs, int32_t bs)
{
    return yuv_clamp((yuv_dot(row, rs, gs, bs) + (128 << 18) + (1 << 17)) >> 18);
}

inline bool yuv_layout_ok(uint32_t layout) { return layout == YUV_I420 || layout == YUV_NV12 || layout == YUV_I444; }

// The bytes of all planes (the layout is a valid one).
inline size_t yuv_bytes(uint32_t W, uint32_t H, uint32_t layout)
{
    const size_t cw = (W + 1u) / 2u, ch = (H + 1u) / 2u;
    return layout == YUV_I444 ? (size_t)3 * W * H : (size_t)W * H + 2u * cw * ch;
}

// The number of planes of a layout, and plane `plane`: its first byte, its width and height in samples and the bytes
// from one sample to the next of the same kind (NV12's second plane: w x h PAIRS, step 2).  false: no such plane.
inline uint32_t yuv_n_planes(uint32_t layout) { return layout == YUV_NV12 ? 2u : 3u; }
inline bool yuv_plane(uint32_t W, uint32_t H, uint32_t layout, uint32_t plane, size_t *offset, uint32_t *w, uint32_t *h, uint32_t *step)
{
    if (plane >= yuv_n_planes(layout)) return false;
    const uint32_t cw = (W + 1u) / 2u, ch = (H + 1u) / 2u;
    const size_t wh = (size_t)W * H;
    if (plane == 0u || layout == YUV_I444) {
        *offset = wh * plane, *w = W, *h = H, *step = 1u;
    } else {
        *offset = wh + (layout == YUV_I420 && plane == 2u ? (size_t)cw * ch : 0u), *w = cw, *h = ch;
        *step = layout == YUV_NV12 ? 2u : 1u;
    }
    return true;
}

// The rule over a whole image on the host (the body of tr_yuv_host; the caller has checked the parameters).  rgb: W x H,
// row 0 = top; out: yuv_bytes, apart from rgb.  Reads every byte of rgb and writes every byte of out, and no other.
inline void yuv_host(uint32_t W, uint32_t H, const uint8_t *rgb, const YuvRule &k, uint8_t *out)
{
    const size_t wh = (size_t)W * H;
    const uint32_t cw = (W + 1u) / 2u, ch = (H + 1u) / 2u;
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t x = 0; x < W; x++) {
            const uint8_t *p = rgb + ((size_t)y * W + x) * 3u;
            out[(size_t)y * W + x] = (uint8_t)yuv_luma(k, p[0], p[1], p[2]);
            if (k.layout == YUV_I444) {
                out[wh + (size_t)y * W + x] = (uint8_t)yuv_chroma1(k.u, p[0], p[1], p[2]);
                out[2u * wh + (size_t)y * W + x] = (uint8_t)yuv_chroma1(k.v, p[0], p[1], p[2]);
            }
        }
    if (k.layout == YUV_I444) return;
    for (uint32_t j = 0; j < ch; j++)
        for (uint32_t i = 0; i < cw; i++) {
            const uint32_t xs[2] = { 2u * i, 2u * i + 1u < W ? 2u * i + 1u : W - 1u };
            const uint32_t ys[2] = { 2u * j, 2u * j + 1u < H ? 2u * j + 1u : H - 1u };
            int32_t s[3] = { 0, 0, 0 };
            for (int a = 0; a < 2; a++)
                for (int b = 0; b < 2; b++)
                    for (int c = 0; c < 3; c++) s[c] += rgb[((size_t)ys[a] * W + xs[b]) * 3u + (size_t)c];
            const uint8_t u = (uint8_t)yuv_chroma4(k.u, s[0], s[1], s[2]), v = (uint8_t)yuv_chroma4(k.v, s[0], s[1], s[2]);
            const size_t at = (size_t)j * cw + i;
            if (k.layout == YUV_NV12) {
                out[wh + 2u * at] = u, out[wh + 2u * at + 1u] = v;
            } else {
                out[wh + at] = u, out[wh + (size_t)cw * ch + at] = v;
            }
        }
}

// k_yuv's arguments, passed by value.  src: width x height rgb8, row 0 = top, tightly packed; clean: null (nothing is
// known: every pixel is read), or the per-tile colour fast-clear flags of src over the whole frame's 128 x 16 tile grid
// (tile row ty holds buffer rows height - 16 (ty + 1) .. height - 1 - 16 ty; ntx flags a tile row); out: yuv_bytes,
// apart from src, any address.
struct YuvArgs {
    const uint8_t *src;
    const uint32_t *clean;
    uint8_t *out;
    uint32_t width, height, ntx;
    YuvRule rule;
};

}  // namespace tr
