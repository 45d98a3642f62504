// tr_lines.h -- the rule of lines (k_lines, tr_lines_host, tr_scene_set_lines' binning): a table of n straight segments,
// n = 0..2^20, is drawn into a finished colour frame F, depth-tested against the frame's own z.  F is W x H, row 0 = top,
// as stored; z is indexed x + y * W, y up (tr_ao.h).  This comment is the contract; the host and the device compile the
// functions below and nothing else.
//   segment  : 32 bytes -- x0, y0 (i32), z0 (f32), x1, y1 (i32), z1 (f32), rgba (four bytes r, g, b, a), reserved (0).
//              Coordinates are the renderer's own raster coordinates (vertex_t_raster): x runs right, y runs UP, pixel
//              (x, y) is frame row H - 1 - y.  Endpoints may lie outside the frame; |x|, |y| <= 2^20; z finite with
//              |z| <= 2^100, so that no step below makes a NaN or an infinity of finite input but the last sum, which
//              may at most overflow to an infinity.
//   pixels   : dx = x1 - x0, dy = y1 - y0; the major axis is x iff |dx| >= |dy|.  The endpoints (with their z) are
//              swapped iff the second one's major coordinate is smaller: a segment and its reverse cover the same pixels.
//              With a the major and b the minor coordinate after the swap, n = a1 - a0 >= 0 and db = b1 - b0, step
//              k = 0..n is major a0 + k, minor b0 + floor((2 k db + n) / (2 n)), an exact floor division (|2 k db + n| <
//              2^44: lines_floor_div); n == 0 is the single pixel (x0, y0).  With `width` w = 1..15 a step covers the minor
//              offsets -((w - 1) / 2) .. +(w / 2) (butt caps).  Pixels outside the frame are dropped.  Every step is a
//              closed form in k: a lane takes a step.
//   depth    : t = (float)k / (float)n, correctly rounded (div_by, tr_math.h; t = 0 if n == 0); z = z0 + (z1 - z0) * t;
//              zl = z + depth_bias: every f32 operation rounded once, nothing contracted.
//   test     : with LINES_DEPTH_TEST a candidate survives at a pixel iff !(zl <= zbuf), the reference's own comparison
//              (shader.rs:175): it survives a NaN depth and f32::MIN (nothing drawn).  Without the flag every candidate
//              survives and no depth is read.
//   winner   : among a pixel's survivors the greatest 64-bit word (key(zl) << 32) | (index + 1) wins, key the total order
//              of tr_stats.h (stats_zkey) over the bits of zl: the nearest candidate, ties to the greatest segment index.
//              With LINES_PAINTER key is 0: the greatest index wins whatever its depth (drawing order).  A maximum does
//              not depend on the order in which candidates arrive.  The word 0 is "no winner" (index + 1 is never 0).
//   output   : only the winner touches the pixel: coverage a = rgba[3] * opacity (opacity 0..256: 0..65280), output
//              layer_mix(rgb, d, a) per channel -- tr_layer.h's NORMAL rule.  A pixel without a winner keeps d.
// Only colour changes: z, winner words and the shadow buffer stay.  A pixel depends on itself and the table alone: the
// rule works in place.
// Binning (the host's, tr_scene_set_lines): a segment enters exactly the 128 x 16 tiles in which one of its pixels AT
// WIDTH 15 lies.  Along the major axis the steps inside one tile column (x major) or tile row (y major) are a range of k;
// the minor coordinate is monotone in k and moves by at most 1 a step, so those steps' pixels cover the minor range
// [min - 7, max + 7] of the range's two ends without a gap, and the tiles that range meets inside the frame are the
// tiles touched: no bounding box, no capacity.  The lists are CSR: offsets[t] .. offsets[t + 1] into `entries`, segment
// indices ascending, t = ty * ntx + tx with tile rows counted up; `tiles` lists the non-empty t ascending.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tr_layer.h"
#include "tr_math.h"
#include "tr_stats.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t LINES_MAX_N = 1u << 20;                         // (= TR_LINES_MAX_N)
constexpr int32_t LINES_COORD_MAX = 1 << 20;                       // |x|, |y|
constexpr uint32_t LINES_MAX_WIDTH = 15u;                          // (= TR_LINES_MAX_WIDTH)
constexpr uint32_t LINES_DEPTH_TEST = 0x1u, LINES_PAINTER = 0x2u;  // (= TR_LINES_DEPTH_TEST, TR_LINES_PAINTER)
constexpr int32_t LINES_BIN_REACH = (int32_t)LINES_MAX_WIDTH / 2;  // the minor offsets of width 15: -7 .. +7
#define TR_LINES_Z_MAX 0x1p100f

// A segment as the table holds it (= tr_line); rgba: r in bits 0..7, g 8..15, b 16..23, alpha 24..31.
struct Line {
    int32_t x0, y0;
    float z0;
    int32_t x1, y1;
    float z1;
    uint32_t rgba, reserved;
};
static_assert(sizeof(Line) == 32, "a segment is 32 bytes");

// The numbers of a call (= tr_lines_params without its reserved words).
struct LinesRule {
    uint32_t width, opacity, flags;
    float bias;
};

// A segment after the swap: major a, minor b; xmajor: a is x.
struct LineGeom {
    int32_t a0, b0, n, db;
    uint32_t xmajor;
    float z0, z1;
};

// Why a segment is refused, or null.
inline const char *lines_refusal(const Line &l)
{
    const int32_t c = LINES_COORD_MAX;
    if (l.x0 < -c || l.x0 > c || l.y0 < -c || l.y0 > c || l.x1 < -c || l.x1 > c || l.y1 < -c || l.y1 > c) return "coordinates must lie within +-2^20";
    if (!(fabsf(l.z0) <= TR_LINES_Z_MAX) || !(fabsf(l.z1) <= TR_LINES_Z_MAX)) return "z must be finite with |z| <= 2^100";
    if (l.reserved != 0u) return "reserved must be 0";
    return nullptr;
}

TR_HD LineGeom lines_geom(const Line &l)
{
    const int32_t dx = l.x1 - l.x0, dy = l.y1 - l.y0;
    const int32_t adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    LineGeom g;
    g.xmajor = adx >= ady ? 1u : 0u;
    const int32_t a0 = g.xmajor ? l.x0 : l.y0, a1 = g.xmajor ? l.x1 : l.y1, b0 = g.xmajor ? l.y0 : l.x0, b1 = g.xmajor ? l.y1 : l.x1;
    const bool swap = a1 < a0;
    g.a0 = swap ? a1 : a0, g.b0 = swap ? b1 : b0;
    g.n = swap ? a0 - a1 : a1 - a0;
    g.db = swap ? b0 - b1 : b1 - b0;
    g.z0 = swap ? l.z1 : l.z0, g.z1 = swap ? l.z0 : l.z1;
    return g;
}

// floor(num / den) for den = 1 .. 2^23 and |num| < 2^45 with a quotient within +-2^30 (the rule's stay within +-2^21):
// the quotient in double is within one of it (both operands are exact doubles), and the remainder, in integers, says
// which way.
TR_HD int32_t lines_floor_div(int64_t num, int32_t den)
{
    int32_t q = (int32_t)floor((double)num / (double)den);
    const int64_t r = num - (int64_t)q * (int64_t)den;
    if (r < 0) q -= 1;
    if (r >= (int64_t)den) q += 1;
    return q;
}

// The minor coordinate of step k = 0..n.
TR_HD int32_t lines_minor(const LineGeom &g, int32_t k)
{
    if (g.n == 0) return g.b0;
    return g.b0 + lines_floor_div(2 * (int64_t)k * (int64_t)g.db + (int64_t)g.n, 2 * g.n);
}

// The divisor of a segment's depth steps.
TR_HD Recip lines_recip(const LineGeom &g) { return recip_of((float)(g.n != 0 ? g.n : 1)); }

// The depth of step k with the bias: what is tested and what orders the candidates.
TR_HD float lines_depth(const LineGeom &g, int32_t k, Recip rn, float bias)
{
    const float t = g.n != 0 ? div_by((float)k, rn) : 0.0f;
    const float dz = g.z1 - g.z0;
    const float m = dz * t;
    const float z = g.z0 + m;
    return z + bias;
}

TR_HD bool lines_survives(float zl, float zbuf) { return !(zl <= zbuf); }

// The word a candidate of segment `index` with depth zl offers to its pixel.
TR_HD uint64_t lines_word(float zl, uint32_t index, uint32_t flags)
{
    const uint32_t key = (flags & LINES_PAINTER) ? 0u : stats_zkey(f32_bits(zl));
    return ((uint64_t)key << 32) | (uint64_t)(index + 1u);
}

// A pixel d (packed) under the winner's word.
TR_HD uint32_t lines_px(uint32_t rgba, uint32_t d, uint32_t opacity) { return layer_px<LAYER_NORMAL>(rgba, d, mul24(rgba >> 24, opacity)); }

// The steps k of a segment whose major coordinate lies in [m0, m1]: *ks .. *ke, empty where *ks > *ke.
TR_HD void lines_steps(const LineGeom &g, int32_t m0, int32_t m1, int32_t *ks, int32_t *ke)
{
    *ks = m0 - g.a0 > 0 ? m0 - g.a0 : 0;
    *ke = m1 - g.a0 < g.n ? m1 - g.a0 : g.n;
}

// f(tx, ty) for every tile a segment's pixels at width 15 touch inside a W x H frame (the header comment says why this
// is exact); tile rows count up.  Each tile is named once: the major ranges are disjoint.
template <typename F>
inline void lines_tiles_of(const LineGeom &g, int32_t W, int32_t H, F f)
{
    const int32_t A = g.xmajor ? W : H, B = g.xmajor ? H : W;            // the frame along the major and the minor axis
    const int32_t TA = g.xmajor ? TILE_W : TILE_H, TB = g.xmajor ? TILE_H : TILE_W;
    int32_t k_lo, k_hi;
    lines_steps(g, 0, A - 1, &k_lo, &k_hi);
    if (k_lo > k_hi) return;
    for (int32_t c = (g.a0 + k_lo) / TA; c <= (g.a0 + k_hi) / TA; c++) {
        int32_t ks, ke;
        lines_steps(g, c * TA, c * TA + TA - 1, &ks, &ke);
        ks = std::max(ks, k_lo), ke = std::min(ke, k_hi);
        const int32_t ba = lines_minor(g, ks), bb = lines_minor(g, ke);
        const int32_t lo = std::max(std::min(ba, bb) - LINES_BIN_REACH, 0), hi = std::min(std::max(ba, bb) + LINES_BIN_REACH, B - 1);
        for (int32_t r = lo / TB; lo <= hi && r <= hi / TB; r++) g.xmajor ? f(c, r) : f(r, c);
    }
}

// The table binned (tr_scene_set_lines; the caller has validated the segments): offsets (n_tiles + 1), entries, tiles.
// Two passes over the segments: the counts, then the entries in segment order, so each list ascends.
inline void lines_bin(uint32_t width, uint32_t height, uint32_t n, const Line *lines, std::vector<uint64_t> &offsets, std::vector<uint32_t> &entries,
                      std::vector<uint32_t> &tiles)
{
    const uint32_t ntx = (width + TILE_W - 1) / TILE_W, nty = (height + TILE_H - 1) / TILE_H;
    offsets.assign((size_t)ntx * nty + 1u, 0u);
    for (uint32_t i = 0; i < n; i++)
        lines_tiles_of(lines_geom(lines[i]), (int32_t)width, (int32_t)height, [&](int32_t tx, int32_t ty) { offsets[(size_t)ty * ntx + (size_t)tx + 1u] += 1u; });
    tiles.clear();
    for (size_t t = 0; t < (size_t)ntx * nty; t++) {
        if (offsets[t + 1] != 0u) tiles.push_back((uint32_t)t);
        offsets[t + 1] += offsets[t];
    }
    entries.assign((size_t)offsets.back(), 0u);
    std::vector<uint64_t> at(offsets.begin(), offsets.end() - 1);
    for (uint32_t i = 0; i < n; i++)
        lines_tiles_of(lines_geom(lines[i]), (int32_t)width, (int32_t)height, [&](int32_t tx, int32_t ty) { entries[(size_t)at[(size_t)ty * ntx + (size_t)tx]++] = i; });
}

// The rule over a whole frame on the host (the body of tr_lines_host; the caller has checked the parameters and the
// segments).  rgb and out: W x H rgb8, row 0 = top; out may be rgb; z (index x + y * W, y up) is read only under
// LINES_DEPTH_TEST.
inline void lines_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const LinesRule &q, uint32_t n, const Line *lines, uint8_t *out)
{
    const int32_t W = (int32_t)width, H = (int32_t)height;
    const int32_t o_lo = -(((int32_t)q.width - 1) / 2), o_hi = (int32_t)q.width / 2;
    std::vector<uint64_t> best((size_t)W * (size_t)H, 0u);
    for (uint32_t i = 0; i < n; i++) {
        const LineGeom g = lines_geom(lines[i]);
        const Recip rn = lines_recip(g);
        int32_t ks, ke;
        lines_steps(g, 0, (g.xmajor ? W : H) - 1, &ks, &ke);
        for (int32_t k = ks; k <= ke; k++) {
            const int32_t bc = lines_minor(g, k);
            const float zl = lines_depth(g, k, rn, q.bias);
            const uint64_t word = lines_word(zl, i, q.flags);
            for (int32_t o = o_lo; o <= o_hi; o++) {
                const int32_t x = g.xmajor ? g.a0 + k : bc + o, y = g.xmajor ? bc + o : g.a0 + k;
                if (x < 0 || x >= W || y < 0 || y >= H) continue;
                const size_t at = (size_t)x + (size_t)y * (size_t)W;
                if ((q.flags & LINES_DEPTH_TEST) && !lines_survives(zl, z[at])) continue;
                if (word > best[at]) best[at] = word;
            }
        }
    }
    if (out != rgb) memmove(out, rgb, (size_t)W * (size_t)H * 3u);
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const uint64_t word = best[(size_t)x + (size_t)y * (size_t)W];
            if (word == 0u) continue;
            uint8_t *o = out + ((size_t)(H - 1 - y) * (size_t)W + (size_t)x) * 3u;
            const uint32_t d = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
            const uint32_t v = lines_px(lines[(uint32_t)word - 1u].rgba, d, q.opacity);
            o[0] = (uint8_t)(v & 0xFFu), o[1] = (uint8_t)((v >> 8) & 0xFFu), o[2] = (uint8_t)((v >> 16) & 0xFFu);
        }
}

// k_lines' arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y; out is fb (in place) or does not
// overlap it, at any byte address.  fbclean: the frame's per-tile colour fast-clear flags (may be null).  z / zclean: only
// under LINES_DEPTH_TEST.  lines, offsets, entries: the table and its CSR lists (32-bit offsets: the caller refuses a
// table with 2^32 entries or more).  tiles: in place, the non-empty tiles, one workgroup each; null out of place, where
// workgroup t takes tile t.  lower: null, or fbclean again -- in place a flagged tile that is stored whole has its flag
// lowered.
struct LinesArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *lower;
    const float *z;
    const uint32_t *zclean;
    const Line *lines;
    const uint32_t *offsets;
    const uint32_t *entries;
    const uint32_t *tiles;
    DevFrame frame;
    LinesRule rule;
};

}  // namespace tr
