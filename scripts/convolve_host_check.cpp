// convolve_host_check.cpp -- the host half of the convolve stage (convolve_host -- the body of tr_convolve_host -- and the
// inline functions k_convolve calls, tr_convolve.h) against a naive double loop in 64-bit integers, over small random
// images and random kernels of both forms up to the bounds, both edge modes, ABS and UNSHARP, plus the copy and the
// constant-frame facts, as a stand-alone program over heap blocks exactly as large as the function may touch.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/convolve_host_check.cpp -o convolve_host_check && ./convolve_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tr_convolve.h"

using namespace tr;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}
static int32_t between(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

static int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// The rule's text, one pixel and channel at a time, in int64.
static uint8_t naive(int64_t W, int64_t H, const uint8_t *rgb, int64_t x, int64_t y, int c, const ConvolveRule &q)
{
    const bool sep = (q.flags & CONVOLVE_SEPARABLE) != 0u;
    const int64_t kw = q.kw, kh = q.kh;
    int64_t acc = 0;
    for (int64_t j = 0; j < kh; j++)
        for (int64_t i = 0; i < kw; i++) {
            const int64_t w = sep ? (int64_t)q.weights[i] * q.weights[kw + j] : q.weights[j * kw + i];
            int64_t sx = x + i - kw / 2, sy = y + j - kh / 2, f;
            if (q.edge == CONVOLVE_CLAMP) sx = clampi(sx, 0, W - 1), sy = clampi(sy, 0, H - 1);
            if (sx < 0 || sx >= W || sy < 0 || sy >= H) f = (q.border >> (8 * c)) & 0xFFu;
            else f = rgb[(sy * W + sx) * 3 + c];
            acc += w * f;
        }
    if (acc + (1ll << 21) >= (1ll << 31) || -acc >= (1ll << 31)) { fprintf(stderr, "the case breaks the bound\n"); exit(2); }
    int64_t v = acc + (q.shift ? 1ll << (q.shift - 1) : 0);
    v = v >= 0 ? v >> q.shift : -((-v + (1ll << q.shift) - 1) >> q.shift);  // floor division: the arithmetic shift
    if ((q.flags & CONVOLVE_ABS) && v < 0) v = -v;
    const int64_t F = rgb[(y * W + x) * 3 + c];
    if (q.flags & CONVOLVE_UNSHARP) {
        v = clampi(v, 0, 255);
        int64_t d = (int64_t)q.amount * (F - v) + 128;
        d = d >= 0 ? d >> 8 : -((-d + 255) >> 8);
        return (uint8_t)clampi(F + d, 0, 255);
    }
    return (uint8_t)clampi(v + q.bias, 0, 255);
}

int main()
{
    int cases = 0;
    for (int round = 0; round < 600; round++) {
        ConvolveRule q;
        memset(&q, 0, sizeof q);
        const bool sep = rnd() % 2u != 0u;
        const int k_max = sep ? CONVOLVE_MAX_SEPARABLE : CONVOLVE_MAX_GENERAL;
        q.kw = 2u * (rnd() % (uint32_t)(k_max / 2 + 1)) + 1u, q.kh = 2u * (rnd() % (uint32_t)(k_max / 2 + 1)) + 1u;
        q.flags = sep ? CONVOLVE_SEPARABLE : 0u;
        const uint32_t kind = rnd() % 4u;
        if (kind == 1u) q.flags |= CONVOLVE_ABS;
        if (kind == 2u) q.flags |= CONVOLVE_UNSHARP, q.amount = rnd() % (CONVOLVE_MAX_AMOUNT + 1u);
        q.shift = rnd() % (CONVOLVE_MAX_SHIFT + 1u);
        q.bias = kind == 2u ? 0 : between(-CONVOLVE_MAX_BIAS, CONVOLVE_MAX_BIAS);
        q.edge = rnd() % 2u;
        q.border = rnd() & 0xFFFFFFu;
        // weights at the bounds: a row of at most 2^15 in absolute sum, a column that keeps A at most 2^22
        const int big = rnd() % 3u == 0u;
        if (sep) {
            const int32_t a = big ? (int32_t)(CONVOLVE_MAX_ROW / q.kw) : 50;
            for (uint32_t i = 0; i < q.kw; i++) q.weights[i] = between(-a, a);
            int64_t row = 0;
            for (uint32_t i = 0; i < q.kw; i++) row += llabs((long long)q.weights[i]);
            if (row == 0) q.weights[0] = 1, row = 1;
            const int64_t b = big ? (CONVOLVE_MAX_A / row) / q.kh : 50;
            const int32_t bb = (int32_t)(b > 32767 ? 32767 : b);
            for (uint32_t j = 0; j < q.kh; j++) q.weights[q.kw + j] = between(-bb, bb);
        } else {
            const int32_t a = big ? 32767 : 300;
            for (uint32_t i = 0; i < q.kw * q.kh; i++) q.weights[i] = big && rnd() % 2u ? (rnd() % 2u ? a : -a) : between(-a, a);
        }
        const int64_t W = between(1, 40), H = between(1, 24);
        uint8_t *rgb = (uint8_t *)malloc((size_t)(W * H * 3)), *out = (uint8_t *)malloc((size_t)(W * H * 3));
        const uint32_t fill = rnd() % 3u;
        for (int64_t i = 0; i < W * H * 3; i++) rgb[i] = fill == 0u ? (uint8_t)rnd() : fill == 1u ? 255 : (uint8_t)(rnd() % 2u * 255u);
        convolve_host((uint32_t)W, (uint32_t)H, rgb, out, q);
        for (int64_t y = 0; y < H; y++)
            for (int64_t x = 0; x < W; x++)
                for (int c = 0; c < 3; c++)
                    if (out[(y * W + x) * 3 + c] != naive(W, H, rgb, x, y, c, q)) {
                        fprintf(stderr, "round %d: (%lld, %lld)[%d] differs\n", round, (long long)x, (long long)y, c);
                        return 1;
                    }
        // the facts: 1 x 1 of weight 1 is a copy
        ConvolveRule one;
        memset(&one, 0, sizeof one);
        one.kw = one.kh = 1u, one.weights[0] = 1, one.flags = sep ? CONVOLVE_SEPARABLE : 0u, one.weights[1] = 1;
        convolve_host((uint32_t)W, (uint32_t)H, rgb, out, one);
        if (memcmp(rgb, out, (size_t)(W * H * 3)) != 0) { fprintf(stderr, "round %d: 1 x 1 is no copy\n", round); return 1; }
        // a box of ones at shift 0 over a constant frame c under CLAMP is min(255, kw * kh * c)
        ConvolveRule box;
        memset(&box, 0, sizeof box);
        box.kw = q.kw, box.kh = q.kh, box.flags = q.flags & CONVOLVE_SEPARABLE, box.edge = CONVOLVE_CLAMP;
        for (uint32_t i = 0; i < (sep ? q.kw + q.kh : q.kw * q.kh); i++) box.weights[i] = 1;
        const uint32_t c = rnd() % 256u, flat = q.kw * q.kh * c < 255u ? q.kw * q.kh * c : 255u;
        memset(rgb, (int)c, (size_t)(W * H * 3));
        convolve_host((uint32_t)W, (uint32_t)H, rgb, out, box);
        for (int64_t i = 0; i < W * H * 3; i++)
            if (out[i] != flat) { fprintf(stderr, "round %d: a box over a constant frame\n", round); return 1; }
        free(rgb), free(out);
        cases++;
    }
    ConvolveRule z;
    memset(&z, 0, sizeof z);
    z.kw = z.kh = 3u, z.bias = -7;
    if (convolve_of_zeros(z) != 0u) return 1;
    z.bias = 200, z.flags = CONVOLVE_ABS;
    if (convolve_of_zeros(z) != 200u) return 1;
    printf("convolve_host_check: %d cases equal the 64-bit loop\n", cases);
    return 0;
}
