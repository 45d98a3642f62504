// distance_host_check.cpp -- the host half of the distance field (distance_host and distance_ramp_host -- the bodies of
// tr_distance_host and tr_distance_ramp_host -- and the inline functions the kernels call, tr_distance.h) against naive
// code in 64-bit integers: the integer square root for EVERY field value; the field over odd sizes, both seed kinds, with
// and without INVERT, against the minimum over all pairs, with R = 255 and single seeds at the frame's corners, where the
// row pass looks four mask words to either side and the column search runs to the frame's edge; the ramp in place and
// out of place over every mode.  Every array is a heap block exactly as large as the function may touch: a byte read or
// written outside it is an error under the sanitizer.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/distance_host_check.cpp -o distance_host_check && ./distance_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tr_distance.h"

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

static float from_bits(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
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

// A frame whose seeds are seed[] (row 0 = top) under either kind: bright with a depth, or dim without.
struct Frame {
    uint32_t W, H;
    uint8_t *rgb, *seed;
    float *z;
};

static Frame make_frame(uint32_t W, uint32_t H)
{
    Frame f = { W, H, (uint8_t *)malloc((size_t)W * H * 3), (uint8_t *)malloc((size_t)W * H), (float *)malloc((size_t)W * H * 4) };
    memset(f.seed, 0, (size_t)W * H);
    return f;
}

static void fill_frame(Frame &f)
{
    for (uint32_t r = 0; r < f.H; r++)
        for (uint32_t x = 0; x < f.W; x++) {
            const size_t i = (size_t)r * f.W + x;
            for (int c = 0; c < 3; c++) f.rgb[3 * i + c] = f.seed[i] ? (uint8_t)(c == 1 ? 200 : rnd() % 200u) : (uint8_t)(rnd() % 100u);
            f.z[x + (size_t)(f.H - 1u - r) * f.W] = f.seed[i] ? (float)(rnd() % 4096u) / 64.0f : from_bits(TR_F32_MIN_BITS);
        }
}

static void free_frame(Frame &f) { free(f.rgb), free(f.seed), free(f.z); }

// The field by all pairs.
static uint16_t naive(const Frame &f, bool invert, uint32_t R, uint32_t x, uint32_t r)
{
    int64_t best = -1;
    for (uint32_t sr = 0; sr < f.H; sr++)
        for (uint32_t sx = 0; sx < f.W; sx++) {
            if ((f.seed[(size_t)sr * f.W + sx] != 0) == invert) continue;
            const int64_t dx = (int64_t)x - sx, dy = (int64_t)r - sr, d = dx * dx + dy * dy;
            if (best < 0 || d < best) best = d;
        }
    return best >= 0 && best <= (int64_t)R * R ? (uint16_t)best : (uint16_t)DIST_FAR;
}

static int check_field(const Frame &f, uint32_t R, long id)
{
    const size_t npx = (size_t)f.W * f.H;
    uint16_t *out = (uint16_t *)malloc(npx * 2);
    for (int form = 0; form < 6; form++) {
        const bool key = form % 3 != 0, invert = form >= 3;
        DistRule q = { key ? DIST_SEED_KEY : DIST_SEED_DRAWN, 200u, R, invert ? DIST_INVERT : 0u };
        distance_host(f.W, f.H, f.rgb, form % 3 == 2 ? nullptr : f.z, q, out);  // (no depth under KEY)
        // every pixel of a small frame; of a large one the rows and columns at its edges and a sample
        for (uint32_t r = 0; r < f.H; r++)
            for (uint32_t x = 0; x < f.W; x++) {
                if (npx > 4096u && r > 1u && r + 2u < f.H && x > 1u && x + 2u < f.W && rnd() % 97u != 0u) continue;
                if (out[(size_t)r * f.W + x] != naive(f, invert, R, x, r)) {
                    free(out);
                    return fail("distance_host", id, (long)x, (long)r);
                }
            }
    }
    free(out);
    return 0;
}

int main()
{
    // the integer square root of d2 << 16 for every field value, and its bounds
    long roots = 0;
    for (uint32_t d2 = 0; d2 <= 65025u; d2++) {
        const uint64_t v = (uint64_t)d2 << 16;
        const uint64_t q = dist_dq(d2);
        if (q * q > v || (q + 1u) * (q + 1u) <= v) return fail("dist_isqrt", (long)d2, (long)q);
        if (q > 65280u) return fail("dq exceeds 65280", (long)d2);
        if ((q * 65536u) >> 32 != 0u) return fail("dq * step leaves a u32", (long)d2);
        if (dist_position_raw(d2, 65536u) != (uint32_t)((q * 65536u) >> 8)) return fail("dist_position_raw", (long)d2);
        roots++;
    }
    for (int k = 0; k < 200000; k++) {  // any u32, too
        const uint32_t v = k < 8 ? 0xFFFFFFFFu - (uint32_t)k : rnd();
        const uint64_t q = dist_isqrt(v);
        if (q * q > v || (q + 1u) * (q + 1u) <= (uint64_t)v) return fail("dist_isqrt of a u32", (long)v);
    }

    // the field: odd sizes and random seeds
    long fields = 0;
    for (int round = 0; round < 40; round++) {
        const uint32_t W = 1u + rnd() % 77u, H = 1u + rnd() % 23u;
        const uint32_t R = round % 4 == 0 ? 255u : round % 4 == 1 ? 1u : 1u + rnd() % 40u;
        Frame f = make_frame(W, H);
        const uint32_t share = round % 5 == 0 ? 2u : 40u;
        for (size_t i = 0; i < (size_t)W * H; i++) f.seed[i] = rnd() % share == 0u;
        if (round == 7) memset(f.seed, 0, (size_t)W * H);
        if (round == 9) memset(f.seed, 1, (size_t)W * H);
        fill_frame(f);
        if (check_field(f, R, round)) return 1;
        free_frame(f);
        fields++;
    }
    // R = 255 and 254 with one seed in a corner of frames wider and taller than the reach, and widths around the mask
    // words' edges
    const uint32_t sizes[][2] = { { 300u, 7u }, { 7u, 300u }, { 257u, 3u }, { 320u, 2u }, { 321u, 1u }, { 1u, 257u }, { 64u, 9u }, { 65u, 9u }, { 129u, 5u } };
    for (const auto &wh : sizes)
        for (int corner = 0; corner < 4; corner++)
            for (uint32_t R = 254u; R <= 255u; R++) {
                Frame f = make_frame(wh[0], wh[1]);
                f.seed[(size_t)(corner / 2 ? wh[1] - 1u : 0u) * wh[0] + (corner % 2 ? wh[0] - 1u : 0u)] = 1;
                fill_frame(f);
                if (check_field(f, R, 1000 + corner)) return 1;
                free_frame(f);
                fields++;
            }

    // the ramp, in place and out of place
    long ramps = 0;
    for (int round = 0; round < 70; round++) {
        const uint32_t W = 1u + rnd() % 33u, H = 1u + rnd() % 13u, n = round % 5 == 0 ? 2u : 2u + rnd() % 63u;
        const size_t npx = (size_t)W * H;
        Frame f = make_frame(W, H);
        for (size_t i = 0; i < npx; i++) f.seed[i] = rnd() % 30u == 0u;
        fill_frame(f);
        uint8_t *out = (uint8_t *)malloc(npx * 3), *in_place = (uint8_t *)malloc(npx * 3), *table = (uint8_t *)malloc((size_t)n * 4);
        uint16_t *field = (uint16_t *)malloc(npx * 2);
        for (size_t i = 0; i < (size_t)n * 4; i++) table[i] = (uint8_t)rnd();
        DistRampRule q = {};
        q.field = { round % 2 ? DIST_SEED_KEY : DIST_SEED_DRAWN, 200u, 1u + rnd() % 9u, round % 3 == 0 ? DIST_INVERT : 0u };
        q.step = round % 4 == 0 ? 65536u : round % 4 == 1 ? 1u : 1u + rnd() % 2000u;
        q.mode = (uint32_t)round % LAYER_MODES, q.opacity = round % 7 == 0 ? 256u : rnd() % 257u;
        q.far = rnd(), q.flags = (uint32_t)(round / 7) % 4u, q.n = n;
        distance_host(W, H, f.rgb, f.z, q.field, field);
        distance_ramp_host(W, H, f.rgb, f.z, q, table, out);
        memcpy(in_place, f.rgb, npx * 3);
        distance_ramp_host(W, H, in_place, f.z, q, table, in_place);
        if (memcmp(in_place, out, npx * 3) != 0) return fail("in place differs from out of place", round);
        for (size_t i = 0; i < npx; i++) {
            int64_t e[4];
            if (field[i] == DIST_FAR) {
                for (int c = 0; c < 4; c++) e[c] = (q.far >> (8 * c)) & 0xFFu;
            } else {
                uint64_t dq = (uint64_t)sqrtl((long double)((uint64_t)field[i] << 16));
                while (dq * dq > ((uint64_t)field[i] << 16)) dq--;
                while ((dq + 1u) * (dq + 1u) <= ((uint64_t)field[i] << 16)) dq++;
                uint64_t p = (dq * q.step) >> 8;
                const uint64_t pmax = (uint64_t)(n - 1u) * 256u;
                p = (q.flags & DIST_REPEAT) ? p % pmax : (p < pmax ? p : pmax);
                const uint64_t a = p >> 8, fr = p & 255u, b = a + 1u < n ? a + 1u : n - 1u;
                for (int c = 0; c < 4; c++) e[c] = (int64_t)((table[4 * a + c] * (256u - fr) + table[4 * b + c] * fr + 128u) >> 8);
            }
            const int64_t cov = ((q.flags & DIST_KEEP_SEEDS) && field[i] == 0u) ? 0 : e[3] * (int64_t)q.opacity;
            for (int c = 0; c < 3; c++) {
                const int64_t d = f.rgb[i * 3 + c];
                const int64_t want = (blend64(q.mode, e[c], d) * cov + d * (65280 - cov) + 32640) / 65280;
                if ((int64_t)out[i * 3 + c] != want) return fail("distance_ramp_host", round, (long)i, c);
            }
        }
        free(out), free(in_place), free(table), free(field);
        free_frame(f);
        ramps++;
    }
    printf("distance: %ld roots, %ld fields, %ld ramps, 0 mismatches\n", roots, fields, ramps);
    return 0;
}
