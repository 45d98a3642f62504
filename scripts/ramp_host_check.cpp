// ramp_host_check.cpp -- the host half of the depth ramp (ramp_host -- the body of tr_ramp_host -- and the inline
// functions k_ramp calls, tr_ramp.h) against naive code in 64-bit integers: the interpolation for EVERY (E_i, E_j, f) with
// its bound, so that two channels share a word without a carry; the position against a restatement in double and u64
// over a sweep of depths, offsets and scales of both signs, the special values included (NaN, +-inf, -0.0, z0 itself,
// f32::MIN, denormals), clamped and under REPEAT; and ramp_host on small random frames over every mode, in place and
// out of place, over heap blocks exactly as large as the function may touch: a byte read or written outside them is an
// error under the sanitizer.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/ramp_host_check.cpp -o ramp_host_check && ./ramp_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tr_ramp.h"

using namespace tr;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

static int fail(const char *what, long a = 0, long b = 0, long c = 0)
{
    printf("FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

static int64_t blend64(uint32_t mode, int64_t s, int64_t d)
{
    switch (mode) {
    case LAYER_ADD: return s + d > 255 ? 255 : s + d;
    case LAYER_MULTIPLY: return (s * d + 127) / 255;
    case LAYER_SCREEN: return 255 - ((255 - s) * (255 - d) + 127) / 255;
    case LAYER_LIGHTEN: return s > d ? s : d;
    case LAYER_DARKEN: return s < d ? s : d;
    case LAYER_DIFFERENCE: return s > d ? s - d : d - s;
    default: return s;
    }
}

// The position in u64: the two f32 steps (volatile: each is stored as an f32), the cast through double.
static uint64_t position64(float z, float z0, float scale, uint32_t n, bool repeat)
{
    volatile float d = z - z0;
    volatile float c = d * scale;
    const double v = (double)c;
    uint64_t p = 0;
    if (v != v || v <= 0.0) p = 0;
    else if (v >= 4294967295.0) p = 4294967295ull;
    else p = (uint64_t)v;
    const uint64_t pmax = (uint64_t)(n - 1u) * 256u;
    return repeat ? p % pmax : (p < pmax ? p : pmax);
}

static float from_bits(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main()
{
    // the interpolation: every pair of bytes and every fraction, in all four channel places of the two words
    long interpolations = 0;
    uint32_t largest = 0;
    for (uint32_t a = 0; a < 256; a++)
        for (uint32_t b = 0; b < 256; b++) {
            const uint32_t table[2] = { a | (b << 8) | (a << 16) | (b << 24), b | (a << 8) | (b << 16) | (a << 24) };
            for (uint32_t f = 0; f < 256; f++) {
                const uint32_t sum_ab = a * (256u - f) + b * f + 128u, sum_ba = b * (256u - f) + a * f + 128u;
                largest = sum_ab > largest ? sum_ab : largest;
                const uint32_t ab = sum_ab >> 8, ba = sum_ba >> 8;
                if (ab > 255u || ba > 255u) return fail("an interpolated channel exceeds a byte", a, b, f);
                const uint32_t want = ab | (ba << 8) | (ab << 16) | (ba << 24);
                if (ramp_entry(table, 2u, f) != want) return fail("ramp_entry", a, b, f);
                interpolations++;
            }
            // f == 0 at the last entry: j is clamped and carries weight 0
            if (ramp_entry(table, 2u, 256u) != table[1]) return fail("ramp_entry at pmax", a, b);
        }
    if (largest != 255u * 256u + 128u || largest >= 65536u) return fail("the interpolation's bound", largest);

    // the position
    const float specials[] = { from_bits(0x7FC00000u), from_bits(0xFFC00001u), INFINITY, -INFINITY, -0.0f, 0.0f, from_bits(TR_F32_MIN_BITS), from_bits(0x7F7FFFFFu),
                               from_bits(1u), from_bits(0x80000001u), 1.0f, -1.0f, 0.25f, 82.0f, 42.0f, 4294967296.0f, 4294967040.0f, 16777216.0f };
    const float z0s[] = { 0.0f, 0.25f, 82.0f, -3.5f, 1.0e30f, -1.0e30f };
    const float scales[] = { 1.0f, -1.0f, 1000.0f, -1632.0f, 65280.0f, -0.001f, 3.0e38f, -3.0e38f, 1.0e-38f };
    const uint32_t ns[] = { 2u, 3u, 17u, 256u, 1024u };
    long positions = 0;
    for (float z0 : z0s)
        for (float scale : scales)
            for (uint32_t n : ns)
                for (int repeat = 0; repeat < 2; repeat++) {
                    RampRule q = {};
                    q.z0 = z0, q.scale = scale, q.n = n, q.flags = repeat ? RAMP_REPEAT : 0u;
                    for (int k = 0; k < 400; k++) {
                        float z;
                        if (k < (int)(sizeof(specials) / sizeof(specials[0]))) z = specials[k];
                        else if (k < 40) z = z0 + (float)(k - 30) * 0.001f;
                        else if (k < 200) z = z0 + ((float)(rnd() % 200001u) - 100000.0f) / (scale * 64.0f);
                        else z = from_bits(rnd());
                        const uint64_t want = position64(z, z0, scale, n, repeat != 0);
                        const uint32_t got = ramp_position(z, q);
                        if ((uint64_t)got != want) return fail("ramp_position", (long)f32_bits(z), (long)got, (long)want);
                        if (got > (n - 1u) * 256u) return fail("a position past pmax", (long)got);
                        positions++;
                    }
                }

    // ramp_host on small frames, in place and out of place
    long frames = 0;
    for (int round = 0; round < 140; round++) {
        const uint32_t W = 1u + rnd() % 19u, H = 1u + rnd() % 9u, n = round % 5 == 0 ? 2u : 2u + rnd() % 63u;
        const size_t npx = (size_t)W * H;
        uint8_t *rgb = (uint8_t *)malloc(npx * 3), *out = (uint8_t *)malloc(npx * 3), *in_place = (uint8_t *)malloc(npx * 3);
        uint8_t *table = (uint8_t *)malloc((size_t)n * 4);
        float *z = (float *)malloc(npx * 4);
        for (size_t i = 0; i < npx * 3; i++) rgb[i] = (uint8_t)rnd();
        for (size_t i = 0; i < (size_t)n * 4; i++) table[i] = (uint8_t)rnd();
        for (uint32_t k = 0; k < n; k++)
            if (rnd() % 4u == 0u) table[4 * k + 3] = rnd() % 2u ? 255 : 0;
        RampRule q = {};
        q.z0 = 0.5f, q.scale = (round % 2 ? -1.0f : 1.0f) * (float)((n - 1u) * 256u) * 2.0f;
        q.mode = (uint32_t)round % LAYER_MODES, q.opacity = round % 7 == 0 ? 256u : rnd() % 257u;
        q.undrawn = rnd(), q.flags = (round / 7) % 2 ? RAMP_REPEAT : 0u, q.n = n;
        for (size_t i = 0; i < npx; i++) {
            const uint32_t pick = rnd() % 8u;
            z[i] = pick == 0u ? from_bits(TR_F32_MIN_BITS) : pick == 1u ? specials[rnd() % 6u] : (float)(rnd() % 4096u) / 4096.0f;
        }
        ramp_host(W, H, rgb, z, q, table, out);
        memcpy(in_place, rgb, npx * 3);
        ramp_host(W, H, in_place, z, q, table, in_place);
        if (memcmp(in_place, out, npx * 3) != 0) return fail("in place differs from out of place", round);
        for (uint32_t r = 0; r < H; r++)
            for (uint32_t x = 0; x < W; x++) {
                const float zz = z[x + (size_t)(H - 1u - r) * W];
                int64_t e[4];
                if (f32_bits(zz) == TR_F32_MIN_BITS) {
                    for (int c = 0; c < 4; c++) e[c] = (q.undrawn >> (8 * c)) & 0xFFu;
                } else {
                    const uint64_t p = position64(zz, q.z0, q.scale, n, (q.flags & RAMP_REPEAT) != 0u);
                    const uint64_t i = p >> 8, f = p & 255u, j = i + 1u < n ? i + 1u : n - 1u;
                    for (int c = 0; c < 4; c++) e[c] = (int64_t)((table[4 * i + c] * (256u - f) + table[4 * j + c] * f + 128u) >> 8);
                }
                const int64_t cov = e[3] * (int64_t)q.opacity;
                for (int c = 0; c < 3; c++) {
                    const int64_t d = rgb[((size_t)r * W + x) * 3 + c];
                    const int64_t want = (blend64(q.mode, e[c], d) * cov + d * (65280 - cov) + 32640) / 65280;
                    if ((int64_t)out[((size_t)r * W + x) * 3 + c] != want) return fail("ramp_host", round, (long)x, (long)r);
                }
            }
        free(rgb), free(out), free(in_place), free(table), free(z);
        frames++;
    }
    printf("ramp: %ld interpolations, %ld positions, %ld frames, 0 mismatches\n", interpolations, positions, frames);
    return 0;
}
