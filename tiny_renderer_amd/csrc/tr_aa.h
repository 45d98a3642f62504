// tr_aa.h -- the rule of edge anti-aliasing (k_aa, tr_aa_host): a luma-driven edge filter of the FXAA family over a
// finished colour frame, at the frame's own size, in integers on the stored bytes.
//
// Orientation and border.  Everything is in the frame BUFFER's orientation: row 0 is the top, y grows downwards, N is
// (x, y - 1), S (x, y + 1), W (x - 1, y), E (x + 1, y).  F(x, y) is the stored rgb8, L(x, y) = stats_luma(F(x, y)), the
// integer BT.709 luma of tr_stats.h, 0..255.  A coordinate outside the frame is clamped to it, x and y each on its own,
// so the border pixel repeats -- for the corners and for q + n of the search as well.
//
// Parameters: contrast_min 0..255, contrast_rel 0..256, search 1..AA_MAX_SEARCH, subpixel 0..256, flags.
//
// For every pixel p = (x, y):
//   1 contrast : M, N, S, W, E the lumas of p and its four neighbours, lo / hi their min / max, range = hi - lo.
//                range < max(contrast_min, (hi * contrast_rel + 128) >> 8), or range == 0: off = 0, p is KEPT.
//   2 direction: EH = |NW + SW - 2 W| + 2 |N + S - 2 M| + |NE + SE - 2 E|
//                EV = |NW + NE - 2 N| + 2 |W + E - 2 M| + |SW + SE - 2 S|;  the edge is horizontal when EH >= EV.
//   3 sides    : horizontal: A = N, B = S, t = (1, 0); vertical: A = W, B = E, t = (0, 1).  gA = |A - M|, gB = |B - M|;
//                the side is A when gA >= gB, else B; g = max(gA, gB); C the chosen neighbour's luma, n the unit step
//                from p to it; mid2 = M + C.
//   4 search   : for s in {-1, +1}, each on its own: k = 1 .. search, q = p + s k t, d2 = L(q) + L(q + n) - mid2, stop
//                at the first k with 2 |d2| >= g.  dist_s = that k, or `search` when none stopped; end_s = the LAST d2
//                evaluated (at k = dist_s either way).  g may be 0 (the contrast lies on the other axis): every d2
//                stops, dist_s = 1.
//   5 edge     : span = dist_- + dist_+ (2..16); the near end is the - end when dist_- < dist_+, else the + end, with
//                `near` its distance and `end` its d2.  good = (end < 0) != (2 M - mid2 < 0).
//                off_e = good ? ((span - 2 near) * 128 + span / 2) / span : 0      (floor divisions; 0..128)
//   6 sub-pixel: a = |2 (N + S + W + E) + NW + NE + SW + SE - 12 M|;  tq = min(256, (a * 256) / (12 * range))
//                sm = (tq * tq * (768 - 2 tq)) >> 16  (0..256);  off_s = (((sm * sm) >> 8) * subpixel) >> 8  (0..256)
//   7 output   : off = max(off_e, off_s), 0..256; per channel (F_p[c] * (256 - off) + F_(p + n)[c] * off + 128) >> 8,
//                p + n clamped like every coordinate.  Under AA_SHOW_BLEND all three channels are min(255, off) -- 0 for
//                a kept pixel --, a diagnostic like TR_DOF_SHOW_COC.
// Decided here where the words leave a choice: the sub-pixel term blends towards the same neighbour p + n as the edge
// term; a pixel whose two ends are equally far takes the + end; `near` is at most span / 2, so off_e is never negative.
//
// A pixel's output depends on lumas within Chebyshev distance `search` and on colours within distance 1: NOT in place.
// Both divisions go through aa_div, a plain u32 division, the same text for both compilers.  One text for the device
// and the host compiler; only where L comes from differs (k_aa: bytes in LDS, staged with the clamp; the host: the
// caller's array through aa_clamp).
#pragma once

#include <stdint.h>

#include <vector>

#include "tr_math.h"
#include "tr_stats.h"
#include "tr_types.h"

namespace tr {

constexpr int AA_MAX_SEARCH = 8;             // (= TR_AA_MAX_SEARCH)
constexpr uint32_t AA_SHOW_BLEND = 0x1u;     // (= TR_AA_SHOW_BLEND)

// The numbers of a call.
struct AaRule {
    uint32_t contrast_min, contrast_rel, search, subpixel, flags;
};

// What aa_found says of a filtered pixel: off in bits 0..8, the neighbour it blends with in bits 9..10.
constexpr uint32_t AA_OFF_MASK = 0x1FFu;
constexpr uint32_t AA_TO_N = 0u, AA_TO_S = 1u, AA_TO_W = 2u, AA_TO_E = 3u;

TR_HD uint32_t aa_luma(uint32_t px) { return stats_luma(px & 0xFFu, (px >> 8) & 0xFFu, (px >> 16) & 0xFFu); }
TR_HD int32_t aa_abs(int32_t v) { return v < 0 ? -v : v; }
TR_HD int32_t aa_clamp(int32_t v, int32_t n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }
TR_HD int32_t aa_dx(uint32_t to) { return to == AA_TO_W ? -1 : to == AA_TO_E ? 1 : 0; }
TR_HD int32_t aa_dy(uint32_t to) { return to == AA_TO_N ? -1 : to == AA_TO_S ? 1 : 0; }

// The rule's two divisions, floor(num / den), den > 0.
TR_HD uint32_t aa_div(uint32_t num, uint32_t den) { return num / den; }

// Step 1: does p pass the contrast test?  *range_out: hi - lo.  (hi * contrast_rel + 128 <= 255 * 256 + 128 < 2^17.)
TR_HD bool aa_passes(int32_t M, int32_t N, int32_t S, int32_t W, int32_t E, const AaRule &q, int32_t *range_out)
{
    int32_t lo = M, hi = M;
    lo = N < lo ? N : lo, hi = N > hi ? N : hi;
    lo = S < lo ? S : lo, hi = S > hi ? S : hi;
    lo = W < lo ? W : lo, hi = W > hi ? W : hi;
    lo = E < lo ? E : lo, hi = E > hi ? E : hi;
    const int32_t range = hi - lo, rel = (int32_t)((mul24((uint32_t)hi, q.contrast_rel) + 128u) >> 8);
    const int32_t need = (int32_t)q.contrast_min > rel ? (int32_t)q.contrast_min : rel;
    *range_out = range;
    return range != 0 && range >= need;
}

// Step 5: the edge term from the span and the near end's distance.  ((span - 2 near) * 128 + span / 2 <= 14 * 128 + 8.)
TR_HD uint32_t aa_edge_offset(uint32_t span, uint32_t near)
{
    return aa_div((span - 2u * near) * 128u + span / 2u, span);
}

// Step 6: tq from a <= 3060 and range 1..255.  (a * 256 <= 783,360 < 2^20.)
TR_HD uint32_t aa_tq(uint32_t a, uint32_t range)
{
    const uint32_t d = aa_div(a * 256u, 12u * range);
    return d < 256u ? d : 256u;
}

// Step 6: the sub-pixel term.  (tq * tq * (768 - 2 tq) is largest at tq = 256: 2^24; sm * sm <= 2^16; (sm * sm >> 8) *
// subpixel <= 2^16.)
TR_HD uint32_t aa_subpixel_offset(uint32_t a, uint32_t range, uint32_t subpixel)
{
    const uint32_t tq = aa_tq(a, range);
    const uint32_t sm = (tq * tq * (768u - 2u * tq)) >> 16;
    return (((sm * sm) >> 8) * subpixel) >> 8;
}

// Steps 2 to 7 of a pixel that passed step 1 with `range`: off | to << 9.  L(x, y): the luma at frame coordinates that
// may lie up to q.search pixels outside the frame (the caller clamps, or has staged the clamp).
template <typename Luma>
TR_HD uint32_t aa_found(const Luma &L, int32_t x, int32_t y, int32_t range, const AaRule &q)
{
    const int32_t M = L(x, y), N = L(x, y - 1), S = L(x, y + 1), W = L(x - 1, y), E = L(x + 1, y);
    const int32_t NW = L(x - 1, y - 1), NE = L(x + 1, y - 1), SW = L(x - 1, y + 1), SE = L(x + 1, y + 1);
    // (every sum of lumas below is at most 12 * 255)
    const int32_t EH = aa_abs(NW + SW - 2 * W) + 2 * aa_abs(N + S - 2 * M) + aa_abs(NE + SE - 2 * E);
    const int32_t EV = aa_abs(NW + NE - 2 * N) + 2 * aa_abs(W + E - 2 * M) + aa_abs(SW + SE - 2 * S);
    const bool horizontal = EH >= EV;
    const int32_t A = horizontal ? N : W, B = horizontal ? S : E;
    const int32_t gA = aa_abs(A - M), gB = aa_abs(B - M);
    const bool side_a = gA >= gB;
    const int32_t g = side_a ? gA : gB, C = side_a ? A : B, mid2 = M + C;
    const uint32_t to = horizontal ? (side_a ? AA_TO_N : AA_TO_S) : (side_a ? AA_TO_W : AA_TO_E);
    const int32_t nx = aa_dx(to), ny = aa_dy(to), tx = horizontal ? 1 : 0, ty = horizontal ? 0 : 1;
    // both directions in one walk: a direction that has stopped keeps its distance and its d2
    const int32_t search = (int32_t)q.search;
    int32_t dist_m = 0, dist_p = 0, end_m = 0, end_p = 0;
    for (int32_t k = 1; k <= search; k++) {
        if (dist_m == 0) {
            const int32_t qx = x - k * tx, qy = y - k * ty;
            end_m = L(qx, qy) + L(qx + nx, qy + ny) - mid2;
            if (2 * aa_abs(end_m) >= g || k == search) dist_m = k;
        }
        if (dist_p == 0) {
            const int32_t qx = x + k * tx, qy = y + k * ty;
            end_p = L(qx, qy) + L(qx + nx, qy + ny) - mid2;
            if (2 * aa_abs(end_p) >= g || k == search) dist_p = k;
        }
        if (dist_m != 0 && dist_p != 0) break;
    }
    const bool minus = dist_m < dist_p;
    const int32_t near = minus ? dist_m : dist_p, end = minus ? end_m : end_p;
    const bool good = (end < 0) != (2 * M - mid2 < 0);
    const uint32_t off_e = good ? aa_edge_offset((uint32_t)(dist_m + dist_p), (uint32_t)near) : 0u;
    const int32_t a = aa_abs(2 * (N + S + W + E) + NW + NE + SW + SE - 12 * M);
    const uint32_t off_s = aa_subpixel_offset((uint32_t)a, (uint32_t)range, q.subpixel);
    return (off_e > off_s ? off_e : off_s) | (to << 9);
}

// Step 7: one channel.  (255 * 256 + 128 < 2^16.)
TR_HD uint32_t aa_channel(uint32_t f, uint32_t fn, uint32_t off) { return (mul24(f, 256u - off) + mul24(fn, off) + 128u) >> 8; }

// Step 7: the pixel, packed (r in bits 0..7, g in 8..15, b in 16..23), from p's and the neighbour's packed colours.
TR_HD uint32_t aa_out_px(uint32_t f, uint32_t fn, uint32_t off, const AaRule &q)
{
    if (q.flags & AA_SHOW_BLEND) {
        const uint32_t v = off < 255u ? off : 255u;
        return v | (v << 8) | (v << 16);
    }
    if (off == 0u) return f;
    return aa_channel(f & 0xFFu, fn & 0xFFu, off) | (aa_channel((f >> 8) & 0xFFu, (fn >> 8) & 0xFFu, off) << 8) |
           (aa_channel((f >> 16) & 0xFFu, (fn >> 16) & 0xFFu, off) << 16);
}

// The luma plane of the host, read through the clamp.
struct AaHostLuma {
    const uint8_t *l;
    int32_t W, H;
    int32_t operator()(int32_t x, int32_t y) const { return (int32_t)l[(size_t)aa_clamp(y, H) * (size_t)W + (size_t)aa_clamp(x, W)]; }
};

// The rule over a whole frame on the host (the body of tr_aa_host; the caller has checked the parameters).  rgb and
// out: row 0 = top, out != rgb.
inline void aa_host(uint32_t width, uint32_t height, const uint8_t *rgb, uint8_t *out, const AaRule &q)
{
    const int32_t W = (int32_t)width, H = (int32_t)height;
    std::vector<uint8_t> luma((size_t)W * (size_t)H);
    auto F = [&](int32_t x, int32_t y) {
        const uint8_t *p = rgb + ((size_t)aa_clamp(y, H) * (size_t)W + (size_t)aa_clamp(x, W)) * 3u;
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    };
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) luma[(size_t)y * (size_t)W + (size_t)x] = (uint8_t)aa_luma(F(x, y));
    const AaHostLuma L = { luma.data(), W, H };
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            int32_t range = 0;
            uint32_t found = 0u;
            if (aa_passes(L(x, y), L(x, y - 1), L(x, y + 1), L(x - 1, y), L(x + 1, y), q, &range)) found = aa_found(L, x, y, range, q);
            const uint32_t off = found & AA_OFF_MASK, to = found >> 9;
            const uint32_t o = aa_out_px(F(x, y), off != 0u ? F(x + aa_dx(to), y + aa_dy(to)) : 0u, off, q);
            uint8_t *d = out + ((size_t)y * (size_t)W + (size_t)x) * 3u;
            d[0] = (uint8_t)(o & 0xFFu), d[1] = (uint8_t)((o >> 8) & 0xFFu), d[2] = (uint8_t)((o >> 16) & 0xFFu);
        }
}

// k_aa's arguments, passed by value.  fb and out: rgb8, row 0 = top (buffer row height - 1 - y of the tile grid's y), out
// does not overlap fb; fbclean: the scene's per-tile colour fast-clear flags over the whole frame's tile grid (band
// scenes are refused; may be null: nothing is known about the colour); out_clean: null, or where the workgroup writes
// the flag of its tile of `out` -- 1: the tile of the frame had its flag up and its output is zeros in every byte.
struct AaArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *out_clean;
    DevFrame frame;
    AaRule rule;
};

}  // namespace tr
