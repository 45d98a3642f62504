// bloom_host_check.cpp -- the host half of bloom (tr_bloom.h: bloom_host -- the body of tr_bloom_host -- and the inline
// functions k_bloom calls) as a stand-alone program, for a run under the host sanitizers.  Needs no GPU and does not
// load the library:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Itiny_renderer_amd/csrc scripts/bloom_host_check.cpp -o bloom_host_check
//   ./bloom_host_check
// It blooms small synthetic images held in arrays exactly as large as the function may touch (1 x 1, 2 x 3, 7 x 5,
// 31 x 33, 64 x 1, 1 x 40 and 130 x 17, so that most taps of the large radii fall outside the frame) at every radius
// 1..15, thresholds 0, 100, 254 and 255, strengths 0, 256 and 1024, plain and with TR_BLOOM_GLOW_ONLY, against a naive
// 2-D double loop in 64-bit integers written from the rule's words, and checks the contract cases: threshold 255 gives
// the frame back; a frame of 255 at strength 1024 stays 255; the sums stay inside u16 / u32.  Exit status 0: all held.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tr_bloom.h"

// The rule as a 2-D sum, per byte.
static void naive(int64_t W, int64_t H, const uint8_t *rgb, uint8_t *out, int64_t R, int64_t thr, int64_t strength, bool glow_only)
{
    const int64_t D = (R + 1) * (R + 1) * (R + 1) * (R + 1);
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++)
            for (int c = 0; c < 3; c++) {
                int64_t V = 0;
                for (int64_t dy = -R; dy <= R; dy++)
                    for (int64_t dx = -R; dx <= R; dx++) {
                        const int64_t qx = x + dx, qy = y + dy;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        const uint8_t *q = rgb + (qy * W + qx) * 3;
                        int64_t m = q[0];
                        if (q[1] > m) m = q[1];
                        if (q[2] > m) m = q[2];
                        if (m > thr) V += (R + 1 - (dx < 0 ? -dx : dx)) * (R + 1 - (dy < 0 ? -dy : dy)) * (int64_t)q[c];
                    }
                const int64_t G = (V + D / 2) / D;
                int64_t o = G;
                if (!glow_only) {
                    o = (int64_t)rgb[(y * W + x) * 3 + c] + ((strength * G + 128) >> 8);
                    if (o > 255) o = 255;
                }
                out[(y * W + x) * 3 + c] = (uint8_t)o;
            }
}

int main()
{
    int bad = 0, cases = 0;
    const uint32_t sizes[][2] = { { 1, 1 }, { 2, 3 }, { 7, 5 }, { 31, 33 }, { 64, 1 }, { 1, 40 }, { 130, 17 } };
    const uint32_t thresholds[] = { 0, 100, 254, 255 }, strengths[] = { 0, 256, 1024 };
    for (const auto &wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        std::vector<uint8_t> rgb(3 * (size_t)W * H), out(rgb.size()), want(rgb.size());
        uint32_t x = 2463534242u + W * 31u + H;
        for (size_t i = 0; i < rgb.size(); i++) {
            x ^= x << 13, x ^= x >> 17, x ^= x << 5;
            // mostly dark with bright speckles, and whole bytes of 255 and 0
            rgb[i] = (x >> 9) % 7u == 0u ? (uint8_t)(200u + (x >> 20) % 56u) : (x >> 9) % 11u == 0u ? 255 : (uint8_t)((x >> 24) % 120u);
        }
        for (uint32_t R = 1; R <= (uint32_t)tr::BLOOM_MAX_RADIUS; R++)
            for (uint32_t thr : thresholds)
                for (uint32_t st : strengths)
                    for (uint32_t glow = 0; glow < 2; glow++) {
                        const tr::BloomRule rule = { R, thr, st, glow };
                        memset(out.data(), 0xEE, out.size());
                        tr::bloom_host(W, H, rgb.data(), out.data(), rule);
                        naive(W, H, rgb.data(), want.data(), R, thr, st, glow != 0u);
                        bad += out != want;
                        if (thr == 255u && !glow) bad += out != rgb;
                        cases++;
                    }
        // saturation: all 255, strength 1024, threshold 0
        std::vector<uint8_t> white(rgb.size(), 255);
        for (uint32_t R = 1; R <= (uint32_t)tr::BLOOM_MAX_RADIUS; R++) {
            const tr::BloomRule rule = { R, 0u, 1024u, 0u };
            tr::bloom_host(W, H, white.data(), out.data(), rule);
            bad += out != white;
            cases++;
        }
    }
    // the sums of a frame of 255 at the largest radius: a horizontal sum of 65280, a sum of both axes of 255 * 65536
    {
        tr::BloomH h = { 0u, 0u };
        for (int d = -15; d <= 15; d++) tr::bloom_h_tap(h, 0xFFFFFFu, tr::bloom_weight(15, d));
        bad += h.rb != (65280u | (65280u << 16)) || h.g != 65280u;
        tr::BloomV v = { 0u, 0u, 0u };
        for (int d = -15; d <= 15; d++) tr::bloom_v_tap(v, h, tr::bloom_weight(15, d));
        bad += v.r != 255u * 65536u || v.g != 255u * 65536u || v.b != 255u * 65536u;
        bad += tr::bloom_glow_px(v, tr::bloom_divisor(15)) != 0xFFFFFFu;
        cases++;
    }
    printf("%d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
