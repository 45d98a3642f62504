// tr_ao.h -- the rule of screen-space ambient occlusion (k_ao, tr_ao_host): a finished colour frame is darkened from its
// own z buffer.  It is the reference's occlusion closure (shader.rs:916-944) moved from the light's shadow buffer to the
// frame's z buffer and from world-space steps to pixel offsets: sixteen samples per ring, the same
// `threshold` / `/ 20.0` / `min(1.0)` form, the same color_blend against black.
//   samples : ring k = 1..rings has radius r_k = (radius * k) / rings (integer division); sample i = 0..15 of it sits at
//             dx = round(fl(r_k * S[i])), dy = round(fl(r_k * C[i])), S / C = sin / cos of 2 pi i / 16 as the f32 literals
//             below, round = half away from zero (Rust's .round()).  Duplicates at small radii are kept and counted.
//   pixel   : z0 = its z; bits(z0) == bits(f32::MIN): not drawn, untouched.  Otherwise, n = 16 * rings,
//             inv_n = fl(1 / n), coef = 1, and for every sample in ring order, i ascending:
//                 zq = z at (x + dx, y + dy); outside the frame, or on a pixel not drawn: f32::MIN
//                 if fl(zq - threshold) > z0:  s = min(fl(fl(zq - z0) / falloff), 1)   (Rust's f32::min: NaN gives 1)
//                                               coef = fl(coef - fl(inv_n * s))
//             channel c -> (fl(fl(coef * c) + fl(fl(1 - coef) * 0))) as u8; with TR_AO_GREY c = 255 in all three.
// Every operation rounds once (the library is built with -ffp-contract=off); a comparison with a NaN is false, so a NaN
// z0 or zq occludes nothing.  One text for the device and the host compiler; only where zq comes from differs (k_ao:
// LDS, the host: the caller's array).
#pragma once

#include <math.h>
#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr int AO_MAX_RADIUS = 16;  // (= TR_AO_MAX_RADIUS)
constexpr int AO_MAX_RINGS = 4;    // (= TR_AO_MAX_RINGS)
constexpr int AO_RING = 16;        // samples per ring
constexpr uint32_t AO_GREY = 1u;   // (= TR_AO_GREY)

// sin and cos of 2 pi i / 16, rounded to f32
#define TR_AO_SIN16 { 0.0f, 0.382683432f, 0.707106781f, 0.923879533f, 1.0f, 0.923879533f, 0.707106781f, 0.382683432f, \
                      0.0f, -0.382683432f, -0.707106781f, -0.923879533f, -1.0f, -0.923879533f, -0.707106781f, -0.382683432f }
#define TR_AO_COS16 { 1.0f, 0.923879533f, 0.707106781f, 0.382683432f, 0.0f, -0.382683432f, -0.707106781f, -0.923879533f, \
                      -1.0f, -0.923879533f, -0.707106781f, -0.382683432f, 0.0f, 0.382683432f, 0.707106781f, 0.923879533f }

// The samples of a call: entry 16 * (k - 1) + i is {dx, dy} of sample i of ring k.  |dx|, |dy| <= radius.
struct AoTaps {
    int8_t d[AO_MAX_RINGS * AO_RING][2];
};

// The table of 16 * rings offsets (1 <= rings <= radius <= AO_MAX_RADIUS, checked by the caller).
TR_HD void ao_offsets(uint32_t radius, uint32_t rings, AoTaps &out)
{
    const float S[AO_RING] = TR_AO_SIN16, C[AO_RING] = TR_AO_COS16;
    for (uint32_t k = 1; k <= rings; k++) {
        const float r = (float)((radius * k) / rings);
        for (int i = 0; i < AO_RING; i++) {
            out.d[AO_RING * (k - 1u) + (uint32_t)i][0] = (int8_t)roundf(r * S[i]);
            out.d[AO_RING * (k - 1u) + (uint32_t)i][1] = (int8_t)roundf(r * C[i]);
        }
    }
}

// The numbers of a call the per-sample step needs.
struct AoRule {
    float threshold, falloff, inv_n;
};

TR_HD AoRule ao_rule(float threshold, float falloff, uint32_t rings)
{
    AoRule r;
    r.threshold = threshold;
    r.falloff = falloff;
    r.inv_n = 1.0f / (float)(AO_RING * rings);
    return r;
}

TR_HD bool ao_drawn(float z0) { return f32_bits(z0) != TR_F32_MIN_BITS; }

// One sample: the pixel's coefficient so far, its own depth z0 and the sample's depth zq.
TR_HD float ao_sample(float coef, float z0, float zq, const AoRule &q)
{
    if (zq - q.threshold > z0) {
        float s = (zq - z0) / q.falloff;
        s = s < 1.0f ? s : 1.0f;  // (f32::min: a NaN gives the other operand)
        coef = coef - q.inv_n * s;
    }
    return coef;
}

// One colour channel under the finished coefficient: color_blend(c, black, coef), util.rs:7-13, as the colour pass has it.
TR_HD uint32_t ao_channel(uint32_t c, float coef) { return blend_black_literal(c, coef); }

// The rule over a whole frame on the host (the body of tr_ao_host; the caller has checked the parameters).  z: index
// x + y * width, y up; rgb: row 0 = top, shaded in place.  Reads width * height floats, reads and writes 3 * width *
// height bytes, nothing else.
inline void ao_host(uint32_t width, uint32_t height, const float *z, uint8_t *rgb, uint32_t radius, uint32_t rings, bool grey,
                    float threshold, float falloff)
{
    AoTaps taps;
    ao_offsets(radius, rings, taps);
    const AoRule rule = ao_rule(threshold, falloff, rings);
    const uint32_t n_taps = (uint32_t)AO_RING * rings;
    const int64_t W = width, H = height;
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            const float z0 = z[x + y * W];
            if (!ao_drawn(z0)) continue;
            float coef = 1.0f;
            for (uint32_t i = 0; i < n_taps; i++) {
                const int64_t qx = x + taps.d[i][0], qy = y + taps.d[i][1];
                const float zq = qx >= 0 && qx < W && qy >= 0 && qy < H ? z[qx + qy * W] : bits_f32(TR_F32_MIN_BITS);
                coef = ao_sample(coef, z0, zq, rule);
            }
            uint8_t *c = rgb + ((H - 1 - y) * W + x) * 3;
            for (int ch = 0; ch < 3; ch++) c[ch] = (uint8_t)ao_channel(grey ? 255u : (uint32_t)c[ch], coef);
        }
}

// k_ao's arguments, passed by value.  z: index x + y * width, y up; colour: rgb8, buffer row height - 1 - y; zclean /
// fbclean: the scene's per-tile fast-clear flags over the whole frame's tile grid (band scenes are refused).
struct AoArgs {
    const float *z;
    const uint32_t *zclean;
    uint8_t *fb;
    uint32_t *fbclean;
    DevFrame frame;
    uint32_t radius, n_taps, grey;
    AoRule rule;
    AoTaps taps;
};

}  // namespace tr
