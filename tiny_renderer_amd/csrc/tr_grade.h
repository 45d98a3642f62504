// tr_grade.h -- the rule of colour grading (k_grade, tr_grade_host): every pixel of a finished colour frame is mapped
// through a 3-D lookup table of N^3 rgb8 colours, N = 2..33, by tetrahedral interpolation in integers.  Red runs fastest
// in the table, the order of a .cube file: the entry for (ir, ig, ib) is number (ib * N + ig) * N + ir.  For a pixel with
// stored channels (vr, vg, vb):
//   split : per channel x: p = v_x * (N - 1);  i_x = p / 255;  f_x = p % 255   (v_x = 255 gives i_x = N - 1, f_x = 0)
//           j_x = min(i_x + 1, N - 1)
//   order : the channels by f, largest first: a, b, c   (f_a >= f_b >= f_c)
//   walk  : V0 = entry(i_r, i_g, i_b);  V1 = V0 with channel a's index stepped to j_a;  V2 = V1 with channel b's index
//           stepped to j_b;  V3 = entry(j_r, j_g, j_b)
//   out   : out[ch] = ((255 - f_a) * V0[ch] + (f_a - f_b) * V1[ch] + (f_b - f_c) * V2[ch] + f_c * V3[ch] + 127) / 255
// The weights are in units of 1 / 255 and sum to 255, so the numerator is at most 255 * 255 + 127 < 2^16: red and blue
// are summed in the two halves of one word without a carry.  NO TIE-BREAK is needed: where two fractions are equal the
// vertex between them has weight 0, so any order of tied channels gives the same bytes.  A clamped j_x (i_x = N - 1)
// goes with f_x = 0 and only ever carries weight 0.  (0, 0, 0) maps to entry 0 exactly -- `c0`, what a cleared tile
// becomes.  Everything is integer and each pixel depends on itself alone: the rule works in place.  One text for the
// device and the host compiler; only where the table lives differs (k_grade: LDS or global memory, one word an entry;
// the host: a vector of such words).
#pragma once

#include <stdint.h>

#include <vector>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t GRADE_MAX_N = 33u;      // (= TR_GRADE_MAX_N)
constexpr uint32_t GRADE_LDS_MAX_N = 25u;  // the largest table k_grade stages into LDS: 25^3 words = 62,500 bytes < 64 KB

static_assert(255u * 255u + 127u < (1u << 16), "a weighted sum of one channel fits a u16");
static_assert(GRADE_LDS_MAX_N * GRADE_LDS_MAX_N * GRADE_LDS_MAX_N * 4u <= 65536u, "the staged table stays below 64 KB");

// The numbers of a call: the table's edge and its entry 0 as a packed pixel.
struct GradeRule {
    uint32_t n, c0;
};

// A pixel and a table entry as the rule sees them: r in bits 0..7, g in 8..15, b in 16..23.
TR_HD uint32_t grade_pack(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// x / 255 for x < 65535 without a multiplication: three full-rate instructions on the device where the compiler's
// multiply-high is a quarter-rate one.  (Every x the rule divides is at most 255 * 255 + 127 = 65152; the stand-alone host
// check compares it with `/` for every x below 65535.)
TR_HD uint32_t grade_div255(uint32_t x) { return (x + 1u + (x >> 8)) >> 8; }

// split: a channel's lower index and its fraction in units of 1 / 255.
struct GradeSplit {
    uint32_t i, f;
};
TR_HD GradeSplit grade_split(uint32_t v, uint32_t n)
{
    const uint32_t p = mul24(v, n - 1u);  // (<= 255 * 32)
    GradeSplit s;
    s.i = grade_div255(p);
    s.f = p - mul24(s.i, 255u);
    return s;
}

// order: (fa, sa) and (fb, sb) exchanged where fa < fb -- a fraction travels with its channel's step through the table.
TR_HD void grade_order(uint32_t &fa, uint32_t &sa, uint32_t &fb, uint32_t &sb)
{
    const bool swap = fa < fb;
    const uint32_t f = swap ? fa : fb, s = swap ? sa : sb;
    fa = swap ? fb : fa, sa = swap ? sb : sa;
    fb = f, sb = s;
}

// One vertex of the walk under weight w: red and blue in the halves of rb, green in g.  (Both factors are below 2^24.)
TR_HD void grade_vertex(uint32_t &rb, uint32_t &g, uint32_t entry, uint32_t w)
{
    rb += mul24(entry & 0x00FF00FFu, w);
    g += mul24((entry >> 8) & 0xFFu, w);
}

// The rule for one packed pixel; lut: N^3 packed entries, wherever they live.
TR_HD uint32_t grade_px(const uint32_t *lut, uint32_t n, uint32_t px)
{
    const GradeSplit r = grade_split(px & 0xFFu, n), g = grade_split((px >> 8) & 0xFFu, n), b = grade_split((px >> 16) & 0xFFu, n);
    // a channel's step to j_x: its stride in the table, or nothing where the index is clamped
    uint32_t f0 = r.f, s0 = r.i + 1u < n ? 1u : 0u;
    uint32_t f1 = g.f, s1 = g.i + 1u < n ? n : 0u;
    uint32_t f2 = b.f, s2 = b.i + 1u < n ? mul24(n, n) : 0u;
    grade_order(f0, s0, f1, s1);
    grade_order(f1, s1, f2, s2);
    grade_order(f0, s0, f1, s1);  // f0 >= f1 >= f2
    const uint32_t at0 = mul24(mul24(b.i, n) + g.i, n) + r.i, at1 = at0 + s0, at2 = at1 + s1, at3 = at2 + s2;
    uint32_t rb = 127u | (127u << 16), gg = 127u;
    grade_vertex(rb, gg, lut[at0], 255u - f0);
    grade_vertex(rb, gg, lut[at1], f0 - f1);
    grade_vertex(rb, gg, lut[at2], f1 - f2);
    grade_vertex(rb, gg, lut[at3], f2);
    return grade_pack(grade_div255(rb & 0xFFFFu), grade_div255(gg), grade_div255(rb >> 16));
}

// The caller's table (3 * n^3 bytes, red fastest) as the packed entries the rule reads.
inline void grade_expand(uint32_t n, const uint8_t *lut, uint32_t *words)
{
    const size_t m = (size_t)n * n * n;
    for (size_t k = 0; k < m; k++) words[k] = grade_pack(lut[3 * k], lut[3 * k + 1], lut[3 * k + 2]);
}

// The rule over n_pixels packed rgb8 pixels on the host (the body of tr_grade_host; the caller has checked n).  out may
// be rgb.  Reads 3 * n_pixels bytes and 3 * n^3 of the table, writes 3 * n_pixels.
inline void grade_host(size_t n_pixels, const uint8_t *rgb, uint8_t *out, uint32_t n, const uint8_t *lut)
{
    std::vector<uint32_t> words((size_t)n * n * n);
    grade_expand(n, lut, words.data());
    for (size_t i = 0; i < n_pixels; i++) {
        const uint32_t o = grade_px(words.data(), n, grade_pack(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]));
        out[3 * i] = (uint8_t)(o & 0xFFu), out[3 * i + 1] = (uint8_t)((o >> 8) & 0xFFu), out[3 * i + 2] = (uint8_t)((o >> 16) & 0xFFu);
    }
}

// k_grade's arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y; out is fb (in place) or does not
// overlap it.  fbclean: the frame's per-tile colour fast-clear flags over the scene's tile grid (a band scene's: its
// band's tiles), read; may be null: nothing is known, every tile is read.  lower_clean: null, or fbclean again -- in
// place with c0 != 0 a flagged tile is stored as c0 and its flag comes down.  lut: n^3 packed entries in device memory.
struct GradeArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *lower_clean;
    const uint32_t *lut;
    DevFrame frame;
    GradeRule rule;
};

}  // namespace tr
