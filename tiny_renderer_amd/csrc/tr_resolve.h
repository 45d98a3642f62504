// tr_resolve.h -- the arithmetic of the supersampling resolve (k_resolve, tr_scene_resolve): a box filter over
// F x F stored u8 values per channel, rounded half up,
//     out = (sum + F*F/2) / (F*F)            (integer; F = 2, 4, 8: the sum fits 14 bits)
// One function for the device and the host compiler, so that both see the same text.
#pragma once

#include <stdint.h>

#include "tr_math.h"

namespace tr {

// One lane's share of the resolve: 16 source pixels (48 bytes = 12 little-endian words) of each of F rows,
// `src[r * 12 + w]`, become 16 / F output pixels, 48 / F bytes packed into `out` (6, 3 or 2 words; unused
// high bytes are zero).  Every index is a constant once the loops are unrolled: byte extracts, 32-bit adds,
// one shift.
template <int F>
TR_HD void resolve_block(const uint32_t *src, uint32_t *out)
{
    static_assert(F == 2 || F == 4 || F == 8, "factor");
    constexpr int N = 16 / F;
    constexpr uint32_t SHIFT = F == 2 ? 2u : F == 4 ? 4u : 6u;  // log2(F * F)
    constexpr int OUT_WORDS = (48 / F + 3) / 4;
#pragma unroll
    for (int w = 0; w < OUT_WORDS; w++) out[w] = 0u;
#pragma unroll
    for (int p = 0; p < N; p++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            uint32_t sum = 0u;
#pragma unroll
            for (int r = 0; r < F; r++) {
#pragma unroll
                for (int dx = 0; dx < F; dx++) {
                    const int b = (p * F + dx) * 3 + c;
                    sum += (src[r * 12 + (b >> 2)] >> (8 * (b & 3))) & 0xFFu;
                }
            }
            const uint32_t v = (sum + (1u << (SHIFT - 1u))) >> SHIFT;
            const int ob = p * 3 + c;
            out[ob >> 2] |= v << (8 * (ob & 3));
        }
    }
}

}  // namespace tr
