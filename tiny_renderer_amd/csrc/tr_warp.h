// tr_warp.h -- the rule of the warp stage (k_warp, tr_warp_host): a frame of W x H rgb8 resampled to W' x H' rgb8 through
// a coarse grid of source coordinates, bilinearly, in integers.  One grid and one kernel for every geometric operation
// -- rotation, flip, lens distortion, keystone, crop-and-zoom, stabilisation, separated colour channels: each is a
// different grid built on the host.  Both images are in the frame BUFFER's orientation (row 0 = top), tightly packed.
//
// Grid.  Nodes are WARP_CELL = 16 output pixels apart: gw = (W' + 15) / 16 + 1 by gh = (H' + 15) / 16 + 1 nodes, row-major,
// each a pair of int32 (sx, sy) in units of 1/256 SOURCE pixel.  256 * x means exactly source sample x: a sample-index
// convention, no half-pixel offset.  Every node value lies in [-2^22, 2^22] (WARP_NODE_MAX); others are refused.
// Coordinate.  Output pixel (X, Y): gx = X >> 4, fx = X & 15, gy = Y >> 4, fy = Y & 15; with n00 = node(gx, gy),
// n10 = node(gx + 1, gy), n01 = node(gx, gy + 1), n11 = node(gx + 1, gy + 1), for sx and sy alike
//     s = ((16 - fx)(16 - fy) n00 + fx (16 - fy) n10 + (16 - fx) fy n01 + fx fy n11 + 128) >> 8
// with an ARITHMETIC shift (floor).  The weights sum to 256 and |n| <= 2^22: everything fits i32.
// Sample.  ix = sx >> 8 (floor), ax = sx & 255, likewise iy, ay;
//     out[c] = ((256 - ax)(256 - ay) T(ix, iy) + ax (256 - ay) T(ix + 1, iy) + (256 - ax) ay T(ix, iy + 1)
//               + ax ay T(ix + 1, iy + 1) + 2^15) >> 16                                   in u32 (<= 255 * 2^16 + 2^15).
// Edge.  WARP_BORDER (0): T is border[c] for a texel outside [0, W) x [0, H).  WARP_CLAMP (1): each texel index is clamped
// to the image.  A texel of weight 0 contributes nothing either way and may be skipped.
// WARP_PER_CHANNEL (flag 1): three grids, r, g, b, gw * gh nodes apart; each channel is sampled at its own coordinate.
// Consequences: the identity grid (node = 256 * 16 * (gx, gy)) at W' x H' = W x H is a copy; sx = 256 * (W - 1 - 16 gx) is
// F[:, ::-1]; a quarter turn is exact; a whole-pixel translation is a shifted copy with border; sx = 128 X doubles the
// width with (a + b + 1) >> 1 midpoints; a constant frame stays constant under WARP_CLAMP.
// The filter is 2 x 2 and no wider: a grid that minifies strongly ALIASES.  Shrink with tr_scene_resize instead.
#pragma once

#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr int WARP_CELL = 16, WARP_CELL_SHIFT = 4;                    // (= TR_WARP_CELL)
constexpr uint32_t WARP_BORDER = 0u, WARP_CLAMP = 1u;                 // (= TR_WARP_BORDER, TR_WARP_CLAMP)
constexpr uint32_t WARP_PER_CHANNEL = 1u;                             // (= TR_WARP_PER_CHANNEL)
constexpr uint32_t WARP_MAX_SIDE = 8192u;
constexpr int32_t WARP_NODE_MAX = 1 << 22;

static_assert((int64_t)WARP_NODE_MAX * 256 + 128 < ((int64_t)1 << 31), "a pixel's coordinate fits i32");
static_assert(255ull * 65536ull + 32768ull < (1ull << 32), "a channel's weighted sum fits u32");

// The numbers of a call.
struct WarpRule {
    uint32_t edge;       // WARP_BORDER or WARP_CLAMP
    uint32_t border[3];  // r, g, b (0..255)
    uint32_t per_channel;
};

TR_HD uint32_t warp_grid_side(uint32_t n) { return (n + (uint32_t)WARP_CELL - 1u) / (uint32_t)WARP_CELL + 1u; }

// One coordinate of a pixel from its cell's four node values.
TR_HD int32_t warp_coord(int32_t n00, int32_t n10, int32_t n01, int32_t n11, int32_t fx, int32_t fy)
{
    return ((16 - fx) * (16 - fy) * n00 + fx * (16 - fy) * n10 + (16 - fx) * fy * n01 + fx * fy * n11 + 128) >> 8;
}

// The four texel weights of a sample's fractions (they sum to 2^16).
struct WarpWeights {
    uint32_t w00, w10, w01, w11;
};
TR_HD WarpWeights warp_weights(uint32_t ax, uint32_t ay)
{
    WarpWeights w;
    w.w00 = (256u - ax) * (256u - ay), w.w10 = ax * (256u - ay), w.w01 = (256u - ax) * ay, w.w11 = ax * ay;
    return w;
}

// The rounding of a channel's weighted sum.
TR_HD uint32_t warp_round(uint32_t sum) { return (sum + (1u << 15)) >> 16; }

// One texel's channel under the edge mode.
inline uint32_t warp_texel_host(uint32_t W, uint32_t H, const uint8_t *rgb, const WarpRule &q, int32_t x, int32_t y, int c)
{
    if (q.edge == WARP_CLAMP) {
        x = x < 0 ? 0 : (x >= (int32_t)W ? (int32_t)W - 1 : x);
        y = y < 0 ? 0 : (y >= (int32_t)H ? (int32_t)H - 1 : y);
    } else if (x < 0 || y < 0 || x >= (int32_t)W || y >= (int32_t)H) {
        return q.border[c];
    }
    return rgb[((size_t)y * W + (size_t)x) * 3u + (size_t)c];
}

// The rule over a whole frame on the host (the body of tr_warp_host; the caller has checked sizes and nodes).  rgb:
// W x H, out: Wd x Hd, both row 0 = top, apart from each other; grid: 1 or 3 grids of 2 * gw * gh int32.
inline void warp_host(uint32_t W, uint32_t H, const uint8_t *rgb, uint32_t Wd, uint32_t Hd, const int32_t *grid, const WarpRule &q, uint8_t *out)
{
    const uint32_t gw = warp_grid_side(Wd), gh = warp_grid_side(Hd);
    const size_t stride = (size_t)gw * gh * 2u;
    for (uint32_t Y = 0; Y < Hd; Y++)
        for (uint32_t X = 0; X < Wd; X++) {
            const uint32_t gx = X >> WARP_CELL_SHIFT, gy = Y >> WARP_CELL_SHIFT;
            const int32_t fx = (int32_t)(X & 15u), fy = (int32_t)(Y & 15u);
            int32_t sx = 0, sy = 0;
            for (int c = 0; c < 3; c++) {
                if (c == 0 || q.per_channel) {
                    const int32_t *g = grid + (q.per_channel ? (size_t)c * stride : 0u);
                    const int32_t *n00 = g + ((size_t)gy * gw + gx) * 2u, *n01 = n00 + (size_t)gw * 2u;
                    sx = warp_coord(n00[0], n00[2], n01[0], n01[2], fx, fy);
                    sy = warp_coord(n00[1], n00[3], n01[1], n01[3], fx, fy);
                }
                const int32_t ix = sx >> 8, iy = sy >> 8;
                const WarpWeights w = warp_weights((uint32_t)(sx & 255), (uint32_t)(sy & 255));
                uint32_t sum = 0u;
                if (w.w00) sum += w.w00 * warp_texel_host(W, H, rgb, q, ix, iy, c);
                if (w.w10) sum += w.w10 * warp_texel_host(W, H, rgb, q, ix + 1, iy, c);
                if (w.w01) sum += w.w01 * warp_texel_host(W, H, rgb, q, ix, iy + 1, c);
                if (w.w11) sum += w.w11 * warp_texel_host(W, H, rgb, q, ix + 1, iy + 1, c);
                out[((size_t)Y * Wd + X) * 3u + (size_t)c] = (uint8_t)warp_round(sum);
            }
        }
}

// k_warp's arguments, passed by value.  fb: the source frame, rgb8, row 0 = top (buffer row height - 1 - y of the tile
// grid's y); fbclean: its per-tile colour fast-clear flags over the whole frame's tile grid (band scenes are refused;
// may be null: nothing is known about the colour); out: out_w x out_h rgb8, apart from fb; grid: the node pairs in device
// memory; out_clean: null, or -- only where out_w x out_h is the frame's size and its height a multiple of 16, so that a
// workgroup's tile IS a tile of the frame's grid -- where each workgroup writes the flag of its tile of `out`.
struct WarpArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *out_clean;
    const int32_t *grid;
    uint32_t out_w, out_h;
    WarpRule rule;
    DevFrame frame;
};

}  // namespace tr
