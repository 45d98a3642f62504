// tr_rank.h -- the rule of the rank stage (k_rank, tr_rank_host): a finished colour frame through an order-statistic
// neighbourhood filter -- median, erode, dilate and what is built from them.  F is the frame as
// tr_scene_get_frame_buffer returns it: rgb8, row 0 = top, y grows downward.
//   footprint : a set of taps inside a kw x kh box, kw and kh odd and 1..15; bit i of rows[j] set: column i from the left,
//               row j from the TOP is a tap.  n taps, n >= 1; rows and columns of the box may be empty, the centre need
//               not be a tap.  Tap (i, j) of pixel (x, y) reads F(x + i - kw / 2, y + j - kh / 2)
//   edge      : a tap outside the image is border[c] under BORDER; under CLAMP its index is clamped per axis
//   ranking   : each channel on its own: the n tap values in ascending order, v(k) is element k, 0-based
//   op        : VALUE v(rank);  RANGE v(rank2) - v(rank);  MID (v(rank) + v(rank2) + 1) >> 1;
//               CLAMP_CENTRE min(max(F(x, y), v(rank)), v(rank2)).  rank <= rank2 <= n - 1; VALUE: rank2 = 0
// Order statistics are exact by nature: every form that selects element k gives the same byte.  A neighbourhood of
// zeros is 0 under every op.  One text for the device and the host compiler.
#pragma once

#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t RANK_VALUE = 0u, RANK_RANGE = 1u, RANK_MID = 2u, RANK_CLAMP_CENTRE = 3u;  // (= TR_RANK_*)
constexpr uint32_t RANK_BORDER = 0u, RANK_CLAMP = 1u;
constexpr uint32_t RANK_MAX_SIDE = 15u, RANK_MAX_TAPS = RANK_MAX_SIDE * RANK_MAX_SIDE;

// tr_rank_params, field for field (tr_scene.cpp asserts the two layouts equal).
struct RankParams {
    uint32_t struct_size, kw, kh, op, rank, rank2, edge;
    uint8_t border[3];
    uint8_t pad;
    uint16_t rows[RANK_MAX_SIDE];
    uint16_t pad2;
};
static_assert(sizeof(RankParams) == 64, "tr_rank_params is 64 bytes");

// The numbers of a call, as the kernel takes them by value.
struct RankRule {
    uint32_t kw, kh, op, rank, rank2, edge;
    uint32_t border;  // r | g << 8 | b << 16
    uint32_t n;       // the number of taps
    uint32_t rows[RANK_MAX_SIDE + 1u];
};

TR_HD uint32_t rank_popcount(uint32_t v)
{
    uint32_t n = 0u;
    for (; v != 0u; v &= v - 1u) n++;
    return n;
}

// The number of taps of a footprint (bits and rows outside the box are the caller's to refuse).
inline uint32_t rank_taps(const RankParams &p)
{
    uint32_t n = 0u;
    for (uint32_t j = 0; j < RANK_MAX_SIDE; j++) n += rank_popcount(p.rows[j]);
    return n;
}

// Why the parameters are refused -- the text behind the entry point's name --, or null.
inline const char *rank_refusal(const RankParams &p)
{
    if (p.struct_size != sizeof(RankParams)) return ": struct_size is not sizeof(tr_rank_params)";
    if (p.kw % 2u == 0u || p.kh % 2u == 0u || p.kw > RANK_MAX_SIDE || p.kh > RANK_MAX_SIDE) return ": kw and kh must be odd and 1..15";
    for (uint32_t j = 0; j < RANK_MAX_SIDE; j++)
        if (j >= p.kh ? p.rows[j] != 0u : (p.rows[j] >> p.kw) != 0u) return ": footprint bits outside the kw x kh box";
    const uint32_t n = rank_taps(p);
    if (n == 0u) return ": the footprint is empty";
    if (p.op > RANK_CLAMP_CENTRE) return ": op must be TR_RANK_VALUE, TR_RANK_RANGE, TR_RANK_MID or TR_RANK_CLAMP_CENTRE";
    if (p.edge != RANK_BORDER && p.edge != RANK_CLAMP) return ": edge must be TR_RANK_BORDER or TR_RANK_CLAMP";
    if (p.pad != 0u || p.pad2 != 0u) return ": pad and pad2 must be 0";
    if (p.rank >= n || p.rank2 >= n) return ": rank and rank2 must be below the number of taps";
    if (p.op == RANK_VALUE && p.rank2 != 0u) return ": rank2 must be 0 under TR_RANK_VALUE";
    if (p.op != RANK_VALUE && p.rank > p.rank2) return ": rank must not exceed rank2";
    return nullptr;
}

// (of parameters that are not refused)
inline RankRule rank_rule(const RankParams &p)
{
    RankRule r = {};
    r.kw = p.kw, r.kh = p.kh, r.op = p.op, r.rank = p.rank, r.edge = p.edge;
    r.rank2 = p.op == RANK_VALUE ? p.rank : p.rank2;  // (one rank: both selections are the same element)
    r.border = (uint32_t)p.border[0] | ((uint32_t)p.border[1] << 8) | ((uint32_t)p.border[2] << 16);
    r.n = rank_taps(p);
    for (uint32_t j = 0; j < RANK_MAX_SIDE; j++) r.rows[j] = p.rows[j];
    return r;
}

// Is column i, row j (from the top) of the box a tap?
TR_HD bool rank_tap(const RankRule &q, uint32_t i, uint32_t j) { return ((q.rows[j] >> i) & 1u) != 0u; }

// op: one channel from v(rank) = lo, v(rank2) = hi (lo <= hi) and the frame's own value F.
TR_HD uint32_t rank_finish(uint32_t op, uint32_t lo, uint32_t hi, uint32_t F)
{
    if (op == RANK_RANGE) return hi - lo;
    if (op == RANK_MID) return (lo + hi + 1u) >> 1;
    if (op == RANK_CLAMP_CENTRE) return F < lo ? lo : F > hi ? hi : F;
    return lo;
}

// The finished pixel from the packed pixels (r | g << 8 | b << 16) of v(rank), v(rank2) and the frame.
TR_HD uint32_t rank_finish_px(uint32_t op, uint32_t lo, uint32_t hi, uint32_t f)
{
    return rank_finish(op, lo & 0xFFu, hi & 0xFFu, f & 0xFFu) | (rank_finish(op, (lo >> 8) & 0xFFu, (hi >> 8) & 0xFFu, (f >> 8) & 0xFFu) << 8) |
           (rank_finish(op, (lo >> 16) & 0xFFu, (hi >> 16) & 0xFFu, (f >> 16) & 0xFFu) << 16);
}

// Element k (0-based, ascending) of the values a histogram counts: a coarse walk over 16 bins of 16 values, then a fine one.
inline uint32_t rank_select(const uint16_t (&coarse)[16], const uint16_t (&fine)[256], uint32_t k)
{
    uint32_t below = 0u, c = 0u;
    while (below + coarse[c] <= k) below += coarse[c++];
    uint32_t v = 16u * c;
    while (below + fine[v] <= k) below += fine[v++];
    return v;
}

// The rule over a whole frame on the host (the body of tr_rank_host; the caller has checked the parameters).  rgb and
// out: row 0 = top, out != rgb.  Reads 3 * width * height bytes, writes as many.  A histogram of the n taps a pixel and
// a channel; the two ranks are read from it.
inline void rank_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out, const RankRule &q)
{
    const int64_t W = width, H = height, kw = q.kw, kh = q.kh, rx = kw / 2, ry = kh / 2;
    const bool clamp = q.edge == RANK_CLAMP;
    const uint8_t border[3] = { (uint8_t)(q.border & 0xFFu), (uint8_t)((q.border >> 8) & 0xFFu), (uint8_t)((q.border >> 16) & 0xFFu) };
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            uint16_t coarse[3][16] = {}, fine[3][256] = {};
            for (int64_t j = 0; j < kh; j++) {
                int64_t yy = y + j - ry;
                const bool y_out = yy < 0 || yy >= H;
                yy = yy < 0 ? 0 : yy >= H ? H - 1 : yy;
                for (int64_t i = 0; i < kw; i++) {
                    if (!rank_tap(q, (uint32_t)i, (uint32_t)j)) continue;
                    int64_t xx = x + i - rx;
                    const bool outside = y_out || xx < 0 || xx >= W;
                    xx = xx < 0 ? 0 : xx >= W ? W - 1 : xx;
                    const uint8_t *t = outside && !clamp ? border : rgb + (yy * W + xx) * 3;
                    for (int c = 0; c < 3; c++) coarse[c][t[c] >> 4]++, fine[c][t[c]]++;
                }
            }
            const uint8_t *f = rgb + (y * W + x) * 3;
            for (int c = 0; c < 3; c++) {
                const uint32_t lo = rank_select(coarse[c], fine[c], q.rank);
                const uint32_t hi = q.rank2 == q.rank ? lo : rank_select(coarse[c], fine[c], q.rank2);
                out[(y * W + x) * 3 + c] = (uint8_t)rank_finish(q.op, lo, hi, f[c]);
            }
        }
}

// k_rank's arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y for the kernel's row y (row 0 =
// bottom), out does not overlap fb; fbclean: the scene's per-tile colour fast-clear flags over the whole frame's tile
// grid (band scenes are refused; may be null: nothing is known about the colour); out_clean: null, or where the
// workgroup writes the flag of its tile of `out`.  words: fb is 4-byte aligned and the width a multiple of 4, so four
// pixels at a multiple of four are three aligned words.
struct RankArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *out_clean;
    DevFrame frame;
    uint32_t words;
    RankRule rule;
};

}  // namespace tr
