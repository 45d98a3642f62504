// tr_stats.h -- the rule of frame statistics (k_stats / k_stats_finish, tr_frame_stats_host, tr_frame_stats_merge): the
// current frame reduced to one record of counts and order statistics.  F is the colour frame as tr_scene_get_frame_buffer
// returns it (row 0 = top), z the depth as tr_scene_read_z_f32 returns it (index x + y * width, y up).  A pixel TAKES PART
// when it lies in the window, the scene's band and the frame.
//   colour (always), per pixel that takes part, over the stored u8 values (R, G, B):
//       hist[0][R]++  hist[1][G]++  hist[2][B]++
//       hist[3][Y]++          Y = (54 R + 183 G + 19 B + 128) >> 8      (integer BT.709; the weights sum to 256)
//       hist[4][max(R, G, B)]++                                          (the key tr_scene_bloom thresholds)
//       n_pixels++
//   depth (TR_STATS_DEPTH), per pixel that takes part and is DRAWN, bits(z) != bits(f32::MIN) (tr_composite.h):
//       n_drawn++;  the box of drawn pixels grows (x0, y0 inclusive, x1, y1 exclusive, output-image coordinates)
//       a NaN z   : n_nan++ and nothing else
//       otherwise : z_min / z_max under the total order of the key k = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000)
//                   (so -0.0 < +0.0), and zhist[min(255, (fl(fl(z - z_lo) * z_scale)) as u32)]++ -- `as u32` is Rust's
//                   cast (f32_to_u32, tr_math.h): truncating, saturating, negatives give 0; -inf lands in bin 0, +inf in 255.
//       No drawn pixel: the box is four zeros.  No drawn pixel that is not NaN: z_min = z_max = f32::MIN.
//   Without the flag every depth field is zero and no depth is looked at.
// Everything is a count or an order statistic: the record does not depend on the order of visits, so the device equals
// the host in every byte, and the record of the union of two disjoint pixel sets follows from the two records alone
// (stats_merge).  Every f32 operation rounds once (the library is built with -ffp-contract=off).  One text for the device
// and the host compiler.
//
// A PARTIAL record (what a k_stats workgroup keeps in LDS and stores to its slot, and what k_stats_finish sums) has the
// record's size and its counts in the record's places; the order statistics are kept as MAXIMA of unsigned words of which
// 0 means "none yet", so that zeros initialise a partial and every field merges by + or by max:
//       zmax = max k          zminc = max ~k         (a key of a non-NaN z is never 0 or 0xFFFFFFFF: those are NaNs)
//       bx1 = max (x + 1)     by1 = max (y + 1)      bx0c = max ~x       by0c = max ~y     (y: output-image row)
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t STATS_DEPTH = 1u;  // (= TR_STATS_DEPTH)
constexpr uint32_t STATS_BINS = 256u;
constexpr uint32_t STATS_HISTS = 5u;  // r, g, b, luma, max channel
constexpr uint32_t STATS_LUMA_R = 54u, STATS_LUMA_G = 183u, STATS_LUMA_B = 19u;

static_assert(STATS_LUMA_R + STATS_LUMA_G + STATS_LUMA_B == 256u, "the luma weights sum to 256");
static_assert(((STATS_LUMA_R + STATS_LUMA_G + STATS_LUMA_B) * 255u + 128u) >> 8 == 255u, "the luma of white is 255: Y <= 255");

// The record (= tr_frame_stats, include/tiny_renderer.h; tr_scene.cpp asserts the two agree).
struct StatsRecord {
    uint32_t hist[STATS_HISTS][STATS_BINS];
    uint32_t zhist[STATS_BINS];
    uint32_t n_pixels, n_drawn, n_nan;
    float z_min, z_max;
    uint32_t box_x0, box_y0, box_x1, box_y1;
    uint32_t reserved[3];
};

// A partial record, word for word over the record: SUMS words that add, then MAXES words that merge by max, then padding.
constexpr uint32_t STATS_WORDS = (uint32_t)(sizeof(StatsRecord) / 4u);
constexpr uint32_t STATS_SUMS = (STATS_HISTS + 1u) * STATS_BINS + 3u;  // the histograms, n_pixels, n_drawn, n_nan
constexpr uint32_t STATS_MAXES = 6u;
enum StatsWord : uint32_t {
    SW_ZHIST = STATS_HISTS * STATS_BINS,
    SW_N_PIXELS = SW_ZHIST + STATS_BINS,
    SW_N_DRAWN,
    SW_N_NAN,
    SW_ZMINC,  // (the place of z_min)
    SW_ZMAX,   // (the place of z_max)
    SW_BX0C,
    SW_BY0C,
    SW_BX1,
    SW_BY1,
    SW_END
};
static_assert(sizeof(StatsRecord) == 6192u && STATS_WORDS == 1548u && STATS_WORDS % 4u == 0u, "the record is 387 16-byte pieces");
static_assert(SW_N_PIXELS == 1536u && SW_N_NAN + 1u == STATS_SUMS && SW_ZMINC == STATS_SUMS && SW_END == STATS_SUMS + STATS_MAXES &&
                  SW_END + 3u == STATS_WORDS,
              "sums, then maxima, then the reserved words");
static_assert(offsetof(StatsRecord, n_pixels) == 4u * SW_N_PIXELS && offsetof(StatsRecord, z_min) == 4u * SW_ZMINC &&
                  offsetof(StatsRecord, z_max) == 4u * SW_ZMAX && offsetof(StatsRecord, box_x0) == 4u * SW_BX0C &&
                  offsetof(StatsRecord, box_y1) == 4u * SW_BY1,
              "a partial's words lie over the record's fields");

// Where the rule looks, in the kernels' coordinates (y up: y = height - 1 - output row): columns [x0, x1), rows [y0, y1),
// already cut to the frame and the band; empty where x0 >= x1 or y0 >= y1.
struct StatsWindow {
    int32_t x0, x1, y0, y1;
};

// The numbers of a call.
struct StatsRule {
    StatsWindow win;
    uint32_t depth;  // TR_STATS_DEPTH given
    float z_lo, z_scale;
};

// The window (x, y, w, h) of output-image coordinates, which lies inside the frame (w == h == 0: all of it), cut to the
// band's rows [band_y0, band_y1) (y up).
inline StatsWindow stats_window(uint32_t width, uint32_t height, uint32_t x, uint32_t y, uint32_t w, uint32_t h, int32_t band_y0,
                                int32_t band_y1)
{
    if (w == 0u && h == 0u) x = 0u, y = 0u, w = width, h = height;
    StatsWindow q;
    q.x0 = (int32_t)x;
    q.x1 = (int32_t)(x + w);
    q.y0 = (int32_t)(height - (y + h));
    q.y1 = (int32_t)(height - y);
    if (q.y0 < band_y0) q.y0 = band_y0;
    if (q.y1 > band_y1) q.y1 = band_y1;
    return q;
}

TR_HD uint32_t stats_luma(uint32_t r, uint32_t g, uint32_t b)
{
    return (mul24(STATS_LUMA_R, r) + mul24(STATS_LUMA_G, g) + mul24(STATS_LUMA_B, b) + 128u) >> 8;
}

TR_HD uint32_t stats_max3(uint32_t r, uint32_t g, uint32_t b)
{
    const uint32_t m = r > g ? r : g;
    return m > b ? m : b;
}

// The key of the total order, and back.
TR_HD uint32_t stats_zkey(uint32_t bits) { return bits ^ ((bits >> 31) != 0u ? 0xFFFFFFFFu : 0x80000000u); }
TR_HD uint32_t stats_zkey_bits(uint32_t key) { return key ^ ((key >> 31) != 0u ? 0x80000000u : 0xFFFFFFFFu); }

TR_HD bool stats_is_nan(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u; }

// The depth histogram's bin of a z that is not NaN.
TR_HD uint32_t stats_zbin(float z, float z_lo, float z_scale)
{
    const float d = z - z_lo;
    const float s = d * z_scale;
    const uint32_t u = f32_to_u32(s);
    return u < STATS_BINS - 1u ? u : STATS_BINS - 1u;
}

// The tail of a partial or a record: words SW_N_PIXELS .. STATS_WORDS - 1.
constexpr uint32_t STATS_TAIL = STATS_WORDS - SW_N_PIXELS;
struct StatsTail {
    uint32_t w[STATS_TAIL];
    TR_HD uint32_t &at(uint32_t word) { return w[word - SW_N_PIXELS]; }
};

// The tail of a finished partial (every slot summed and maxed) turned into the record's public form in place.  depth:
// TR_STATS_DEPTH was given -- without it z_min and z_max are zeros like every depth field, not f32::MIN.
TR_HD void stats_publish(StatsTail &t, bool depth)
{
    const bool any_z = t.at(SW_N_DRAWN) > t.at(SW_N_NAN);
    const bool any = t.at(SW_N_DRAWN) != 0u;
    const uint32_t none = depth ? TR_F32_MIN_BITS : 0u;
    t.at(SW_ZMINC) = any_z ? stats_zkey_bits(~t.at(SW_ZMINC)) : none;
    t.at(SW_ZMAX) = any_z ? stats_zkey_bits(t.at(SW_ZMAX)) : none;
    t.at(SW_BX0C) = any ? ~t.at(SW_BX0C) : 0u;
    t.at(SW_BY0C) = any ? ~t.at(SW_BY0C) : 0u;
    t.at(SW_BX1) = any ? t.at(SW_BX1) : 0u;
    t.at(SW_BY1) = any ? t.at(SW_BY1) : 0u;
    t.at(SW_END) = t.at(SW_END + 1u) = t.at(SW_END + 2u) = 0u;
}

// Was the record made without TR_STATS_DEPTH?  (With it, a record in which nothing is drawn holds f32::MIN, never zeros.)
inline bool stats_colour_only(StatsTail &t) { return t.at(SW_N_DRAWN) == 0u && t.at(SW_ZMINC) == 0u && t.at(SW_ZMAX) == 0u; }

// ... and a record's tail back into a partial's (stats_merge), in place.
inline void stats_unpublish(StatsTail &t)
{
    const bool any_z = t.at(SW_N_DRAWN) > t.at(SW_N_NAN);
    const bool any = t.at(SW_N_DRAWN) != 0u;
    t.at(SW_ZMINC) = any_z ? ~stats_zkey(t.at(SW_ZMINC)) : 0u;
    t.at(SW_ZMAX) = any_z ? stats_zkey(t.at(SW_ZMAX)) : 0u;
    t.at(SW_BX0C) = any ? ~t.at(SW_BX0C) : 0u;
    t.at(SW_BY0C) = any ? ~t.at(SW_BY0C) : 0u;
    if (!any) t.at(SW_BX1) = t.at(SW_BY1) = 0u;
}

// The same over the tail of a whole partial / record held as words.
inline void stats_publish_words(uint32_t *w, bool depth)
{
    StatsTail t;
    memcpy(t.w, w + SW_N_PIXELS, sizeof t.w);
    stats_publish(t, depth);
    memcpy(w + SW_N_PIXELS, t.w, sizeof t.w);
}
inline bool stats_unpublish_words(uint32_t *w)  // (returns stats_colour_only)
{
    StatsTail t;
    memcpy(t.w, w + SW_N_PIXELS, sizeof t.w);
    const bool colour_only = stats_colour_only(t);
    stats_unpublish(t);
    memcpy(w + SW_N_PIXELS, t.w, sizeof t.w);
    return colour_only;
}

// Partial b into partial a.
inline void stats_fold(uint32_t *a, const uint32_t *b)
{
    for (uint32_t i = 0; i < STATS_SUMS; i++) a[i] += b[i];
    for (uint32_t i = STATS_SUMS; i < SW_END; i++) a[i] = a[i] > b[i] ? a[i] : b[i];
}

// One pixel into a partial on the host: colour (r, g, b); with `z` non-null its depth at output-image place (x, row).
inline void stats_pixel_host(uint32_t *w, const StatsRule &q, uint32_t r, uint32_t g, uint32_t b, const float *z, uint32_t x, uint32_t row)
{
    w[0u * STATS_BINS + r] += 1u;
    w[1u * STATS_BINS + g] += 1u;
    w[2u * STATS_BINS + b] += 1u;
    w[3u * STATS_BINS + stats_luma(r, g, b)] += 1u;
    w[4u * STATS_BINS + stats_max3(r, g, b)] += 1u;
    w[SW_N_PIXELS] += 1u;
    if (!z) return;
    const uint32_t bits = f32_bits(*z);
    if (bits == TR_F32_MIN_BITS) return;
    w[SW_N_DRAWN] += 1u;
    if (~x > w[SW_BX0C]) w[SW_BX0C] = ~x;
    if (~row > w[SW_BY0C]) w[SW_BY0C] = ~row;
    if (x + 1u > w[SW_BX1]) w[SW_BX1] = x + 1u;
    if (row + 1u > w[SW_BY1]) w[SW_BY1] = row + 1u;
    if (stats_is_nan(bits)) {
        w[SW_N_NAN] += 1u;
        return;
    }
    const uint32_t k = stats_zkey(bits);
    if (k > w[SW_ZMAX]) w[SW_ZMAX] = k;
    if (~k > w[SW_ZMINC]) w[SW_ZMINC] = ~k;
    w[SW_ZHIST + stats_zbin(*z, q.z_lo, q.z_scale)] += 1u;
}

// The rule over a frame on the host (the body of tr_frame_stats_host; the caller has checked the parameters).  rgb: row 0 =
// top; z (read only when q.depth): index x + y * width, y up.  Reads the window's pixels, writes *out, nothing else.
inline void stats_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const StatsRule &q, StatsRecord *out)
{
    uint32_t w[STATS_WORDS];
    memset(w, 0, sizeof w);
    for (int32_t y = q.win.y0; y < q.win.y1; y++) {
        const uint32_t row = height - 1u - (uint32_t)y;
        for (int32_t x = q.win.x0; x < q.win.x1; x++) {
            const uint8_t *c = rgb + ((size_t)row * width + (size_t)x) * 3u;
            stats_pixel_host(w, q, c[0], c[1], c[2], q.depth ? z + (size_t)y * width + (size_t)x : nullptr, (uint32_t)x, row);
        }
    }
    stats_publish_words(w, q.depth != 0u);
    memcpy(out, w, sizeof w);
}

// The record of the union of two disjoint pixel sets (the body of tr_frame_stats_merge): src into dst.
inline void stats_merge(StatsRecord *dst, const StatsRecord *src)
{
    uint32_t a[STATS_WORDS], b[STATS_WORDS];
    memcpy(a, dst, sizeof a);
    memcpy(b, src, sizeof b);
    const bool ca = stats_unpublish_words(a), cb = stats_unpublish_words(b);
    stats_fold(a, b);
    stats_publish_words(a, !(ca && cb));
    memcpy(dst, a, sizeof a);
}

// k_stats' arguments, passed by value.  fb: rgb8, buffer row height - 1 - y.  fbclean / zclean: the frame's per-tile
// fast-clear flags over the scene's tile grid (a band scene's: its band's tiles), read; fbclean may be null: nothing is
// known, every tile is read.  z, zclean: read only when rule.depth and not `cleared`.  cleared: the scene is logically
// cleared -- every tile counts as flagged in both arrays and nothing is loaded.  partials: one slot of STATS_WORDS words a
// workgroup, each stored whole.
struct StatsArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    const float *z;
    const uint32_t *zclean;
    uint32_t *partials;
    DevFrame frame;
    StatsRule rule;
    uint32_t cleared;
};

}  // namespace tr
