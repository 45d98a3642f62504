// tr_resize.h -- the rule of the resize stage (k_resize, tr_resize_host, tr_resize_taps): a frame of W x H rgb8 scaled
// to W' x H' rgb8 by a separable filter with integer weights, in the frame BUFFER's orientation (row 0 = top).  The two
// axes are independent; what follows speaks of ONE axis with N source and M output samples.
//
// Raw taps.  Output index X gets raw integer taps o[x] over the source indices x in [0, N):
//   RESIZE_AREA (0)     o[x] = max(0, min((x + 1) M, (X + 1) N) - max(x M, X N)): the overlap of the two pixels'
//                       intervals in units of 1 / (N M);
//   RESIZE_BILINEAR (1) a triangle whose support grows with the ratio when minifying: S = 2 max(M, N), C = (2 X + 1) N,
//                       o[x] = max(0, S - |(2 x + 1) M - C|).  Taps that would fall outside [0, N) are DROPPED, not
//                       clamped; the normalisation makes up for them.
// Normalisation.  The taps with o[x] > 0 form one run x0 .. x0 + n - 1.  Their weights sum to exactly 4096 by cumulative
// rounding: O = sum of o, cum_k = o[x0] + .. + o[x0 + k], c_k = (4096 cum_k + O / 2) / O (integer division in 64 bits),
// w_k = c_k - c_(k-1) with c_(-1) = 0.  A weight may come out 0 and is kept.
// Output.  out[Y][X][c] = ( sum_j wy[Y][j] * ( sum_k wx[X][k] * F[y0(Y) + j][x0(X) + k][c] ) + 2^23 ) >> 24.  The inner
// sum is not rounded and is at most 255 * 4096; the outer sum plus 2^23 is at most 255 * 2^24 + 2^23 < 2^32: u32.
// Limits.  ceil(N / 8) <= M <= RESIZE_MAX_SIDE per axis (a minification beyond 8 is refused; a magnification is bounded
// by the size alone).  Within them a run holds at most 9 (area) or 16 (bilinear) taps: RESIZE_MAX_TAPS.
//
// The divisions above are evaluated on the HOST only (resize_axis): the device gets, per axis, a table of first index
// and tap count and a table of weights, RESIZE_MAX_TAPS to an output index and zero beyond the count, and k_resize
// multiplies and adds.  resize_host is the rule over a caller's array through the same tables.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "tr_types.h"

namespace tr {

constexpr uint32_t RESIZE_AREA = 0u, RESIZE_BILINEAR = 1u;  // (= TR_RESIZE_AREA, TR_RESIZE_BILINEAR)
constexpr int RESIZE_MAX_TAPS = 16;                         // (= TR_RESIZE_MAX_TAPS)
constexpr uint32_t RESIZE_MAX_SIDE = 8192u;
constexpr uint32_t RESIZE_ONE = 4096u;  // the sum of a run's weights

// One raw tap (the caller keeps x in [0, N)).
inline int64_t resize_raw(uint32_t filter, int64_t N, int64_t M, int64_t X, int64_t x)
{
    if (filter == RESIZE_AREA) return std::max<int64_t>(0, std::min((x + 1) * M, (X + 1) * N) - std::max(x * M, X * N));
    const int64_t S = 2 * std::max(M, N), C = (2 * X + 1) * N, d = (2 * x + 1) * M - C;
    return std::max<int64_t>(0, S - (d < 0 ? -d : d));
}

// Is n_dst an output size the rule allows for n_src source samples?
inline bool resize_side_ok(uint32_t n_src, uint32_t n_dst)
{
    return n_src >= 1u && n_dst >= 1u && n_dst <= RESIZE_MAX_SIDE && (uint64_t)n_dst * 8u >= (uint64_t)n_src;
}

// The tables of one axis: first[X], count[X] and weights[X * RESIZE_MAX_TAPS + k] (zeros for k >= count[X]).  The
// largest count goes to *max_count (may be null).  false: a run longer than RESIZE_MAX_TAPS (not within the limits).
inline bool resize_axis(uint32_t filter, uint32_t n_src, uint32_t n_dst, uint16_t *first, uint16_t *count, uint16_t *weights, uint32_t *max_count)
{
    const int64_t N = (int64_t)n_src, M = (int64_t)n_dst;
    uint32_t most = 0u;
    for (int64_t X = 0; X < M; X++) {
        // a lower bound of the run's first index, then a walk: area, x + 1 > X N / M; bilinear, (2 x + 1) M > C - S
        int64_t x = filter == RESIZE_AREA ? (X * N) / M : 0;
        if (filter != RESIZE_AREA) {
            const int64_t t = (2 * X + 1) * N - 2 * std::max(M, N);
            x = t <= 0 ? 0 : std::max<int64_t>(0, t / (2 * M) - 1);
        }
        while (x < N && resize_raw(filter, N, M, X, x) == 0) x++;
        int64_t o[RESIZE_MAX_TAPS], O = 0;
        int n = 0;
        for (; x + n < N; n++) {
            const int64_t v = resize_raw(filter, N, M, X, x + n);
            if (v == 0) break;
            if (n == RESIZE_MAX_TAPS) return false;
            o[n] = v;
            O += v;
        }
        if (n == 0) return false;
        first[X] = (uint16_t)x;
        count[X] = (uint16_t)n;
        int64_t cum = 0, before = 0;
        for (int k = 0; k < RESIZE_MAX_TAPS; k++) {
            uint16_t w = 0u;
            if (k < n) {
                cum += o[k];
                const int64_t c = ((int64_t)RESIZE_ONE * cum + O / 2) / O;
                w = (uint16_t)(c - before);
                before = c;
            }
            weights[(size_t)X * RESIZE_MAX_TAPS + (size_t)k] = w;
        }
        most = std::max(most, (uint32_t)n);
    }
    if (max_count) *max_count = most;
    return true;
}

// The tables of one axis, owned.
struct ResizeAxis {
    std::vector<uint16_t> first, count, weights;
    uint32_t max_count = 0u;
    bool build(uint32_t filter, uint32_t n_src, uint32_t n_dst)
    {
        first.assign(n_dst, 0u);
        count.assign(n_dst, 0u);
        weights.assign((size_t)n_dst * RESIZE_MAX_TAPS, 0u);
        return resize_axis(filter, n_src, n_dst, first.data(), count.data(), weights.data(), &max_count);
    }
    // The most source samples that `group` consecutive output indices, starting at a multiple of `group`, reach over.
    uint32_t span(uint32_t group) const
    {
        uint32_t most = 0u;
        const uint32_t M = (uint32_t)first.size();
        for (uint32_t a = 0; a < M; a += group) {
            const uint32_t b = std::min(a + group, M) - 1u;
            most = std::max(most, (uint32_t)first[b] + (uint32_t)count[b] - (uint32_t)first[a]);
        }
        return most;
    }
};

// The rule over a whole frame on the host (the body of tr_resize_host; the caller has checked the sizes).  rgb: W x H,
// out: W' x H', both row 0 = top, apart from each other.
inline bool resize_host(uint32_t W, uint32_t H, const uint8_t *rgb, uint32_t filter, uint32_t Wd, uint32_t Hd, uint8_t *out)
{
    ResizeAxis ax, ay;
    if (!ax.build(filter, W, Wd) || !ay.build(filter, H, Hd)) return false;
    std::vector<uint32_t> rows((size_t)H * Wd * 3u);  // the horizontal sums of every source row
    for (uint32_t y = 0; y < H; y++)
        for (uint32_t X = 0; X < Wd; X++) {
            uint32_t acc[3] = { 0u, 0u, 0u };
            const uint8_t *p = rgb + ((size_t)y * W + ax.first[X]) * 3u;
            for (uint32_t k = 0; k < ax.count[X]; k++)
                for (int c = 0; c < 3; c++) acc[c] += (uint32_t)ax.weights[(size_t)X * RESIZE_MAX_TAPS + k] * p[3u * k + (uint32_t)c];
            for (int c = 0; c < 3; c++) rows[((size_t)y * Wd + X) * 3u + (size_t)c] = acc[c];
        }
    for (uint32_t Y = 0; Y < Hd; Y++)
        for (uint32_t j = 0; j < Wd * 3u; j++) {
            uint32_t acc = 1u << 23;
            for (uint32_t k = 0; k < ay.count[Y]; k++)
                acc += (uint32_t)ay.weights[(size_t)Y * RESIZE_MAX_TAPS + k] * rows[(size_t)(ay.first[Y] + k) * Wd * 3u + j];
            out[(size_t)Y * Wd * 3u + j] = (uint8_t)(acc >> 24);
        }
    return true;
}

// The compiled shapes of k_resize: a workgroup's tile of the OUTPUT is w x h pixels, and the source rows its h output
// rows reach over -- at most `rows` -- hold their horizontal sums in LDS (rows * w * 12 bytes).  The launcher's caller
// takes the first shape whose `rows` the vertical table's span(h) fits (resize_shape); the last one fits every table
// within the limits: 4 output rows reach over at most 5 * 8 + 1 source rows.
struct ResizeShape {
    int w, h, rows;
};
constexpr int RESIZE_SHAPES = 3;
constexpr ResizeShape kResizeShapes[RESIZE_SHAPES] = { { 64, 16, 24 }, { 32, 8, 40 }, { 32, 4, 48 } };

// The shape for a vertical table, or -1.
inline int resize_shape(const ResizeAxis &ay)
{
    for (int i = 0; i < RESIZE_SHAPES; i++)
        if (ay.span((uint32_t)kResizeShapes[i].h) <= (uint32_t)kResizeShapes[i].rows) return i;
    return -1;
}

// An axis's tables in device memory: fc[X] = first | count << 16, w[X * RESIZE_MAX_TAPS + k] (16-byte aligned).
struct ResizeTable {
    const uint32_t *fc;
    const uint16_t *w;
};

// k_resize's arguments, passed by value.  fb: the source frame, rgb8, row 0 = top (buffer row height - 1 - y of the tile
// grid's y); fbclean: its per-tile colour fast-clear flags over the whole frame's tile grid (band scenes are refused;
// may be null: nothing is known about the colour); out: out_w x out_h rgb8, apart from fb.
struct ResizeArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t out_w, out_h;
    ResizeTable x, y;
    int shape;        // of kResizeShapes, from resize_shape
    uint32_t y_span;  // the vertical table's span(kResizeShapes[shape].h)
    uint32_t x_span;  // the horizontal table's span(kResizeShapes[shape].w)
    DevFrame frame;
};

}  // namespace tr
