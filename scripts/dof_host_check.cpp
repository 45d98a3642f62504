// dof_host_check.cpp -- the host half of depth of field (tr_dof.h: dof_coc_host -- the body of tr_dof_coc --, dof_host --
// the body of tr_dof_host --, dof_div) as a stand-alone program, for a run under the host sanitizers.  Needs no GPU and
// does not load the library:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Itiny_renderer_amd/csrc scripts/dof_host_check.cpp -o dof_host_check
//   ./dof_host_check
// It blurs small synthetic fields held in arrays exactly as large as the functions may touch (37 x 29, 1 x 1 and 3 x 64,
// so that most taps fall outside the frame), at every radius with the background circle 0 and at the radius, plain and
// with TR_DOF_SHOW_COC, with NaN, infinities and undrawn pixels in the field, and checks the contract cases: NaN gives
// circle 0, an infinity max_radius, an undrawn pixel background_radius; a frame whose circles are all 0 comes back byte
// for byte; a constant colour stays constant; the division by reciprocal and correction equals `/`.  Exit status 0: all
// held.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tr_dof.h"

int main()
{
    int bad = 0;
    const float z_min = tr::bits_f32(TR_F32_MIN_BITS);
    // the division: every sw a frame can reach is a sum of at most 289 table weights; sampled sums, every quotient
    // 0..255 at the edges of its interval
    {
        uint32_t x = 12345u;
        for (int k = 0; k < 200000; k++) {
            x = x * 1664525u + 1013904223u;
            uint32_t sw = 0;
            const int taps = 1 + (int)((x >> 8) % 289u);
            uint32_t y = x;
            for (int t = 0; t < taps; t++) {
                y = y * 1664525u + 1013904223u;
                sw += tr::dof_weight((y >> 16) % 9u);
            }
            const float inv = 1.0f / (float)sw;
            const uint32_t q = (x >> 3) % 256u;
            const uint32_t ns[4] = { q * sw, q * sw + sw - 1u, q * sw + (sw >> 1), q == 255u ? q * sw + (sw >> 1) : q * sw + sw };
            for (uint32_t n : ns) bad += tr::dof_div(n, sw, inv) != n / sw;
        }
    }
    const uint32_t sizes[][2] = { { 37, 29 }, { 1, 1 }, { 3, 64 } };
    for (uint32_t R = 1; R <= (uint32_t)tr::DOF_MAX_RADIUS; R++)
        for (int back = 0; back < 2; back++)
            for (const auto &wh : sizes) {
                const uint32_t W = wh[0], H = wh[1];
                const tr::DofRule rule = { 100.0f, 2.0f, 0.5f, R, back ? R : 0u };
                std::vector<float> z((size_t)W * H);
                std::vector<uint8_t> rgb(3 * (size_t)W * H), out(rgb.size()), coc(z.size());
                for (uint32_t y = 0; y < H; y++)
                    for (uint32_t x = 0; x < W; x++) {
                        const size_t i = x + (size_t)y * W;
                        z[i] = 100.0f + 30.0f * sinf(0.7f * (float)x) * cosf(0.4f * (float)y);
                        if (i % 11 == 3) z[i] = z_min;
                        if (i % 53 == 7) z[i] = NAN;
                        if (i % 59 == 9) z[i] = INFINITY;
                        if (i % 61 == 11) z[i] = -INFINITY;
                    }
                for (size_t i = 0; i < rgb.size(); i++) rgb[i] = (uint8_t)(i * 37u + 11u);
                tr::dof_coc_host(rule, (uint32_t)z.size(), z.data(), coc.data());
                for (size_t i = 0; i < z.size(); i++) {
                    bad += coc[i] > R;
                    if (tr::f32_bits(z[i]) == TR_F32_MIN_BITS) bad += coc[i] != rule.background_radius;
                    else if (isnan(z[i])) bad += coc[i] != 0;
                    else if (isinf(z[i])) bad += coc[i] != R;
                }
                for (int show = 0; show < 2; show++) {
                    memset(out.data(), 0xEE, out.size());
                    tr::dof_host(W, H, z.data(), rgb.data(), out.data(), rule, show != 0);
                    if (show)
                        for (uint32_t y = 0; y < H; y++)
                            for (uint32_t x = 0; x < W; x++)
                                bad += out[3 * ((size_t)(H - 1 - y) * W + x)] != coc[x + (size_t)y * W] * 255u / R;
                }
                // a constant colour stays constant under any circles
                std::vector<uint8_t> flat(rgb.size(), 201);
                tr::dof_host(W, H, z.data(), flat.data(), out.data(), rule, false);
                bad += out != flat;
                // every circle 0: the frame byte for byte
                for (float &v : z) v = 101.5f;
                tr::dof_host(W, H, z.data(), rgb.data(), out.data(), rule, false);
                bad += out != rgb;
            }
    // a white pixel of circle 1 beside a black one of circle 0: (255 * 3640 + (3640 + 32768) / 2) / (3640 + 32768) = 25
    {
        const tr::DofRule rule = { 0.0f, 0.0f, 1.0f, 8u, 0u };
        const float z[2] = { 1.0f, 0.0f };
        const uint8_t rgb[6] = { 255, 255, 255, 0, 0, 0 };
        uint8_t out[6];
        tr::dof_host(2, 1, z, rgb, out, rule, false);
        bad += out[0] != 255 || out[3] != 25 || out[4] != 25 || out[5] != 25;
        printf("right pixel %u (25 expected)\n", out[3]);
    }
    printf("%d mismatches\n", bad);
    return bad ? 1 : 0;
}
