// tr_accumulate.h -- the rule of frame accumulation (k_accumulate, tr_accumulate_host): n kept frames of one call are
// averaged under integer weights, byte by byte on their stored u8 values (no gamma), rounded half up:
//     D = sum of w_k,   out[b] = (sum of w_k * F_k[b] + D / 2) / D        (integer division)
// with 1 <= n <= 32, 0 <= w_k <= 255 and D >= 1, so D <= 8160 and the numerator stays below
// 255 * 8160 + 4080 + 1 = 2 084 881 < 2^21.  A frame of weight 0 contributes nothing (and is never read).
// The division is a multiplication: with l = floor(log2 D) and m = ceil(2^(23 + l) / D) <= 2^24,
//     num / D = (num * m) >> (23 + l)           for every num < 2^21
// (e = m * D - 2^(23 + l) < D < 2^(l + 1), and the quotient is exact while num * e < 2^(23 + l): 2^21 * 2^(l + 1) is).
// The device takes the product's high word: ((num << 11) * m) >> 32 >> (l + 2) -- one shift, one 32 x 32 high
// multiplication, one shift, no division.  One function for the device and the host compiler, so that both see the same
// text.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t ACC_MAX_FRAMES = 32;  // (= TR_ACCUMULATE_MAX_FRAMES)
constexpr uint32_t ACC_MAX_WEIGHT = 255;
constexpr uint32_t ACC_MAX_DIVISOR = ACC_MAX_FRAMES * ACC_MAX_WEIGHT;               // 8160
constexpr uint32_t ACC_MAX_NUMERATOR = 255u * ACC_MAX_DIVISOR + ACC_MAX_DIVISOR / 2u;  // 2 084 880 < 2^21

// The divisor of a call as the per-byte step needs it (accumulate_divisor makes one).
struct AccDiv {
    uint32_t half;   // D / 2, the rounding term
    uint32_t mul;    // ceil(2^(23 + l) / D), l = floor(log2 D)
    uint32_t shift;  // l + 2
};

// 1 <= D <= ACC_MAX_DIVISOR (checked by the caller).
TR_HD AccDiv accumulate_divisor(uint32_t D)
{
    uint32_t l = 0;
    while ((D >> (l + 1u)) != 0u) l++;
    const uint64_t p = (uint64_t)1 << (23u + l);
    AccDiv d;
    d.half = D / 2u;
    d.mul = (uint32_t)((p + D - 1u) / D);
    d.shift = l + 2u;
    return d;
}

// num / D for num <= ACC_MAX_NUMERATOR (num << 11 fits 32 bits).
TR_HD uint32_t accumulate_div(uint32_t num, const AccDiv &d)
{
    return (uint32_t)(((uint64_t)(num << 11) * (uint64_t)d.mul) >> 32) >> d.shift;
}

// What k_accumulate gets.  Frame k's colour buffer fb[k], its colour-clean flags clean[k] (one word per tile of the
// band; null: nothing known, the tile is read) and its weight w[k]; `out` is the destination, out_clean its flags when
// it is one of the frames (in place), else null.
struct AccumulateArgs {
    const uint8_t *fb[ACC_MAX_FRAMES];
    const uint32_t *clean[ACC_MAX_FRAMES];
    uint8_t *out;
    uint32_t *out_clean;
    DevFrame frame;
    uint32_t n;
    AccDiv div;
    uint32_t w[ACC_MAX_FRAMES];
};

// The rule over n_bytes bytes of n frames on the host.  Weights and divisor as above (checked by the caller).
inline void accumulate_host(size_t n_bytes, uint32_t n, const uint8_t *const *frames, const uint32_t *weights, uint8_t *out)
{
    uint32_t D = 0;
    for (uint32_t k = 0; k < n; k++) D += weights ? weights[k] : 1u;
    const AccDiv d = accumulate_divisor(D);
    for (size_t b = 0; b < n_bytes; b++) {
        uint32_t num = d.half;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t w = weights ? weights[k] : 1u;
            if (w != 0u) num += w * (uint32_t)frames[k][b];
        }
        out[b] = (uint8_t)accumulate_div(num, d);
    }
}

}  // namespace tr
