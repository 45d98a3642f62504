// bilateral_host_check.cpp -- the host half of the bilateral stage (bilateral_host -- the body of tr_bilateral_host --, the
// parameter check and the inline functions k_bilateral shares, tr_bilateral.h) against naive 64-bit code, over small
// random and extreme images, windows, range tables, both guides and both edge modes; the accumulator bound (all 225
// taps at weight 255 x 255 on value 255); the depth distance at NaN, the infinities, f32::MIN and a scale of 0; and the
// refusals, as a stand-alone program over heap blocks exactly as large as the function may touch.  The finish is a plain
// u32 division, so there is no reciprocal to prove exact.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/bilateral_host_check.cpp -o bilateral_host_check && ./bilateral_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <limits>

#include "tr_bilateral.h"

using namespace tr;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}
static int32_t between(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }
static int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

static const float kMin = -std::numeric_limits<float>::max();

// The rule's text for the depth distance, in double where the f32 operations allow it: the difference and the product
// are each rounded to f32 once (volatile keeps the compiler from carrying more).
static uint32_t naive_depth_distance(float zt, float zc, float scale)
{
    volatile float diff = zt - zc;
    volatile float t = fabsf(diff) * scale;
    if (isnan(t) || !(t < 255.0f)) return 255u;
    return (uint32_t)(double)t;
}

// The rule's text, one pixel at a time, in 64 bits.
static void naive(int64_t W, int64_t H, const uint8_t *rgb, const float *z, int64_t x, int64_t y, const BilateralParams &p, uint8_t (&o)[3])
{
    uint64_t S = 0, A[3] = { 0, 0, 0 };
    const uint8_t *C = rgb + (y * W + x) * 3;
    for (int64_t j = 0; j < p.kh; j++)
        for (int64_t i = 0; i < p.kw; i++) {
            const uint64_t sw = p.spatial[j * p.kw + i];
            if (sw == 0) continue;
            int64_t sx = x + i - p.kw / 2, sy = y + j - p.kh / 2;
            if (p.edge == BILATERAL_CLAMP) sx = clampi(sx, 0, W - 1), sy = clampi(sy, 0, H - 1);
            const bool outside = sx < 0 || sx >= W || sy < 0 || sy >= H;
            const uint8_t *T = outside ? p.border : rgb + (sy * W + sx) * 3;
            uint32_t d = 0;
            if (p.guide == BILATERAL_GUIDE_COLOUR) {
                for (int c = 0; c < 3; c++) d = (uint32_t)llabs((long long)T[c] - (long long)C[c]) > d ? (uint32_t)llabs((long long)T[c] - (long long)C[c]) : d;
            } else {
                const float zt = outside ? kMin : z[(H - 1 - sy) * W + sx];
                d = naive_depth_distance(zt, z[(H - 1 - y) * W + x], p.depth_scale);
            }
            const uint64_t w = sw * p.range[d];
            S += w;
            for (int c = 0; c < 3; c++) A[c] += w * T[c];
        }
    for (int c = 0; c < 3; c++) o[c] = S == 0 ? C[c] : (uint8_t)((A[c] + S / 2) / S);
}

static bool refused(const BilateralParams &p, const char *why)
{
    const char *got = bilateral_refusal(p);
    return got != nullptr && strcmp(got, why) == 0;
}

static BilateralParams blank(uint32_t kw, uint32_t kh)
{
    BilateralParams p;
    memset(&p, 0, sizeof p);
    p.struct_size = sizeof p, p.kw = kw, p.kh = kh;
    return p;
}

static int compare(int round, int64_t W, int64_t H, const uint8_t *rgb, const float *z, const BilateralParams &p)
{
    uint8_t *out = (uint8_t *)malloc((size_t)(W * H * 3));
    bilateral_host((uint32_t)W, (uint32_t)H, rgb, p.guide == BILATERAL_GUIDE_DEPTH ? z : nullptr, out, bilateral_rule(p));
    int bad = 0;
    for (int64_t y = 0; y < H && !bad; y++)
        for (int64_t x = 0; x < W && !bad; x++) {
            uint8_t want[3];
            naive(W, H, rgb, z, x, y, p, want);
            if (memcmp(out + (y * W + x) * 3, want, 3) != 0) {
                fprintf(stderr, "round %d: (%lld, %lld) differs\n", round, (long long)x, (long long)y);
                bad = 1;
            }
        }
    free(out);
    return bad;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    int cases = 0;
    for (int round = 0; round < 400; round++) {
        BilateralParams p = blank(2u * (rnd() % 8u) + 1u, 2u * (rnd() % 8u) + 1u);
        const uint32_t density = rnd() % 4u, heavy = rnd() % 3u;  // density 0: every tap; heavy 0: every weight 255
        for (uint32_t k = 0; k < p.kw * p.kh; k++)
            if (density == 0u || rnd() % (density + 1u) == 0u) p.spatial[k] = heavy == 0u ? 255 : (uint8_t)(1u + rnd() % 255u);
        if (rnd() % 5u == 0u) p.spatial[(p.kh / 2u) * p.kw + p.kw / 2u] = 0;  // a centre that is no tap
        bool any = false;
        for (uint32_t k = 0; k < p.kw * p.kh; k++) any = any || p.spatial[k] != 0;
        if (!any) p.spatial[rnd() % (p.kw * p.kh)] = 255;
        const uint32_t table = rnd() % 5u;  // all 255, a step, random, all zeros, a falling ramp
        const uint32_t cut = rnd() % 40u;
        for (uint32_t d = 0; d < 256u; d++)
            p.range[d] = table == 0u ? 255 : table == 1u ? (d <= cut ? 255 : 0) : table == 2u ? (uint8_t)rnd() : table == 3u ? 0 : (uint8_t)(255u - d);
        p.guide = rnd() % 2u, p.edge = rnd() % 2u;
        p.depth_scale = rnd() % 6u == 0u ? 0.0f : (float)(rnd() % 4000u) / 16.0f;
        p.border[0] = (uint8_t)rnd(), p.border[1] = (uint8_t)rnd(), p.border[2] = (uint8_t)rnd();
        if (bilateral_refusal(p) != nullptr) { fprintf(stderr, "round %d: refused: %s\n", round, bilateral_refusal(p)); return 1; }
        const int64_t W = between(1, 36), H = between(1, 22);
        uint8_t *rgb = (uint8_t *)malloc((size_t)(W * H * 3));
        float *z = (float *)malloc((size_t)(W * H) * sizeof(float));
        const uint32_t fill = rnd() % 4u;  // noise, white, black and white, a narrow band of noise
        for (int64_t i = 0; i < W * H * 3; i++)
            rgb[i] = fill == 0u ? (uint8_t)rnd() : fill == 1u ? 255 : fill == 2u ? (uint8_t)(rnd() % 2u * 255u) : (uint8_t)(100u + rnd() % 12u);
        for (int64_t i = 0; i < W * H; i++) {
            const uint32_t kind = rnd() % 16u;
            z[i] = kind == 0u ? kMin : kind == 1u ? nan : kind == 2u ? (rnd() % 2u ? inf : -inf) : -10.0f + (float)(rnd() % 2048u) / 1024.0f;
        }
        if (compare(round, W, H, rgb, z, p)) return 1;
        // the facts: a centre-only window and an all-zero range table are the identity
        uint8_t *out = (uint8_t *)malloc((size_t)(W * H * 3));
        BilateralParams one = p;
        memset(one.spatial, 0, sizeof one.spatial);
        one.spatial[(p.kh / 2u) * p.kw + p.kw / 2u] = (uint8_t)(1u + rnd() % 255u);
        bilateral_host((uint32_t)W, (uint32_t)H, rgb, z, out, bilateral_rule(one));
        BilateralParams none = p;
        memset(none.range, 0, sizeof none.range);
        bool identity = true;
        // (a centre whose own distance is 255 -- a NaN depth -- under range[255] == 0 has S == 0: the centre again)
        if (memcmp(rgb, out, (size_t)(W * H * 3)) != 0) identity = false;
        bilateral_host((uint32_t)W, (uint32_t)H, rgb, z, out, bilateral_rule(none));
        if (memcmp(rgb, out, (size_t)(W * H * 3)) != 0) identity = false;
        if (!identity) { fprintf(stderr, "round %d: an identity is none\n", round); return 1; }
        free(rgb), free(z), free(out);
        cases++;
    }
    // the accumulator bound: all 225 taps at weight 255 x 255 on value 255
    {
        BilateralParams p = blank(15u, 15u);
        memset(p.spatial, 255, sizeof p.spatial);
        memset(p.range, 255, sizeof p.range);
        p.edge = BILATERAL_CLAMP;
        const int64_t W = 17, H = 16;
        uint8_t *rgb = (uint8_t *)malloc((size_t)(W * H * 3)), *out = (uint8_t *)malloc((size_t)(W * H * 3));
        float *z = (float *)malloc((size_t)(W * H) * sizeof(float));
        memset(rgb, 255, (size_t)(W * H * 3));
        for (int64_t i = 0; i < W * H; i++) z[i] = -3.0f;
        for (uint32_t guide = 0; guide < 2u; guide++) {
            p.guide = guide;
            bilateral_host((uint32_t)W, (uint32_t)H, rgb, z, out, bilateral_rule(p));
            for (int64_t i = 0; i < W * H * 3; i++)
                if (out[i] != 255) { fprintf(stderr, "the bound: byte %lld is %u\n", (long long)i, out[i]); return 1; }
            if (compare(-1, W, H, rgb, z, p)) return 1;
        }
        BilateralSums m = { 0u, { 0u, 0u, 0u } };
        for (uint32_t k = 0; k < BILATERAL_MAX_TAPS; k++) bilateral_tap(m, 65025u, 0xFFFFFFu);
        if (m.s != 14630625u || m.a[0] != 3730809375u || m.a[1] != m.a[0] || m.a[2] != m.a[0] || (uint64_t)m.a[0] + m.s / 2u != 3738124687ull ||
            bilateral_finish_px(m, 0u) != 0xFFFFFFu)
            return 1;
        // rounding of the finish: halves go up
        BilateralSums h = { 2u, { 1u, 2u, 3u } };
        if (bilateral_finish_px(h, 0u) != (1u | (1u << 8) | (2u << 16))) return 1;
        BilateralSums zero = { 0u, { 0u, 0u, 0u } };
        if (bilateral_finish_px(zero, 0x123456u) != 0x123456u) return 1;
        free(rgb), free(out), free(z);
    }
    // the depth distance
    {
        struct { float zt, zc, scale; uint32_t d; } facts[] = {
            { nan, -3.0f, 10.0f, 255u }, { -3.0f, nan, 10.0f, 255u }, { nan, nan, 10.0f, 255u }, { nan, nan, 0.0f, 255u },
            { inf, -3.0f, 1.0f, 255u }, { -3.0f, -inf, 1.0f, 255u }, { inf, inf, 1.0f, 255u }, { inf, -3.0f, 0.0f, 255u },
            { kMin, -3.0f, 1.0f, 255u }, { -3.0f, kMin, 1.0f, 255u }, { kMin, kMin, 1.0f, 0u }, { kMin, kMin, 3.0e38f, 0u },
            { kMin, -3.0f, 0.0f, 0u }, { kMin, -3.0f, 1.0e-37f, 34u }, { kMin, 3.0e38f, 1.0f, 255u },
            { -9.0f, -10.0f, 100.0f, 100u }, { -10.0f, -9.0f, 100.0f, 100u }, { -10.0f, -10.0f, 100.0f, 0u }, { -9.0f, -10.0f, 0.0f, 0u },
            { -9.0f, -10.0f, 254.99f, 254u }, { -9.0f, -10.0f, 255.0f, 255u }, { -9.0f, -10.0f, 3.0e38f, 255u }, { 0.0f, -0.0f, 5.0f, 0u },
        };
        for (const auto &f : facts) {
            const uint32_t got = bilateral_depth_distance(f.zt, f.zc, f.scale);
            if (got != f.d || naive_depth_distance(f.zt, f.zc, f.scale) != f.d) {
                fprintf(stderr, "distance(%g, %g, %g) = %u, the text says %u\n", (double)f.zt, (double)f.zc, (double)f.scale, got, f.d);
                return 1;
            }
        }
        for (int k = 0; k < 200000; k++) {
            uint32_t a = rnd(), b = rnd(), c = rnd() & 0x7FFFFFFFu;
            float zt, zc, scale;
            memcpy(&zt, &a, 4), memcpy(&zc, &b, 4), memcpy(&scale, &c, 4);
            if (!(scale <= 3.402823466e38f)) continue;
            if (bilateral_depth_distance(zt, zc, scale) != naive_depth_distance(zt, zc, scale)) { fprintf(stderr, "distance of bits %08x %08x %08x\n", a, b, c); return 1; }
        }
        if (bilateral_colour_distance(0x00FF00u, 0xFF00FFu) != 255u || bilateral_colour_distance(0x102030u, 0x122530u) != 5u || bilateral_colour_distance(7u, 7u) != 0u) return 1;
    }
    // the refusals, each with its text
    BilateralParams ok = blank(3u, 3u);
    memset(ok.spatial, 9, 9);
    ok.range[0] = 1;
    if (bilateral_refusal(ok) != nullptr) return 1;
    BilateralParams w = ok;
    w.struct_size = 508u;
    if (!refused(w, ": struct_size is not sizeof(tr_bilateral_params)")) return 1;
    w = ok, w.kw = 4u;
    if (!refused(w, ": kw and kh must be odd and 1..15")) return 1;
    w = ok, w.kh = 17u;
    if (!refused(w, ": kw and kh must be odd and 1..15")) return 1;
    w = ok, w.spatial[9] = 1;
    if (!refused(w, ": spatial weights outside the kw x kh window")) return 1;
    w = ok, w.spatial[224] = 1;
    if (!refused(w, ": spatial weights outside the kw x kh window")) return 1;
    w = ok, memset(w.spatial, 0, sizeof w.spatial);
    if (!refused(w, ": the window is all zeros")) return 1;
    w = ok, w.guide = 2u;
    if (!refused(w, ": guide must be TR_BILATERAL_GUIDE_COLOUR or TR_BILATERAL_GUIDE_DEPTH")) return 1;
    w = ok, w.edge = 2u;
    if (!refused(w, ": edge must be TR_BILATERAL_BORDER or TR_BILATERAL_CLAMP")) return 1;
    for (float bad : { -1.0f, inf, -inf, nan }) {
        w = ok, w.depth_scale = bad;
        if (!refused(w, ": depth_scale must be finite and >= 0")) return 1;
    }
    w = ok, w.depth_scale = -0.0f;
    if (bilateral_refusal(w) != nullptr) return 1;
    w = ok, w.depth_scale = 3.402823466e38f;
    if (bilateral_refusal(w) != nullptr) return 1;
    w = ok, w.pad = 1;
    if (!refused(w, ": pad and pad2 must be 0")) return 1;
    for (int k = 0; k < 3; k++) {
        w = ok, w.pad2[k] = 1;
        if (!refused(w, ": pad and pad2 must be 0")) return 1;
    }
    printf("bilateral_host_check: %d cases equal the 64-bit rule\n", cases);
    return 0;
}
