// ao_host_check.cpp -- the host half of ambient occlusion (tr_ao.h: ao_offsets, ao_host -- the body of tr_ao_host) as a
// stand-alone program, for a run under the host sanitizers.  Needs no GPU and does not load the library:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Itiny_renderer_amd/csrc scripts/ao_host_check.cpp -o ao_host_check
//   ./ao_host_check
// It shades small synthetic fields held in arrays exactly as large as the function may touch (37 x 29 and 1 x 1, so
// that most samples fall outside the frame), at every radius with every ring count, plain and grey, with NaN, infinities
// and undrawn pixels in the field, and checks the contract cases: the sample table stays inside the radius, an undrawn
// pixel keeps its bytes, a flat field is left alone, a pixel under a step is darkened.  Exit status 0: all held.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tr_ao.h"

int main()
{
    int bad = 0;
    const float z_min = tr::bits_f32(TR_F32_MIN_BITS);
    for (uint32_t radius = 1; radius <= (uint32_t)tr::AO_MAX_RADIUS; radius++)
        for (uint32_t rings = 1; rings <= (uint32_t)tr::AO_MAX_RINGS && rings <= radius; rings++) {
            tr::AoTaps taps;
            memset(&taps, 0x7F, sizeof taps);
            tr::ao_offsets(radius, rings, taps);
            int reach = 0;
            for (uint32_t i = 0; i < 16u * rings; i++) {
                const int dx = taps.d[i][0], dy = taps.d[i][1];
                bad += abs(dx) > (int)radius || abs(dy) > (int)radius;
                reach = abs(dx) > reach ? abs(dx) : reach;
            }
            bad += reach != (int)radius;
            const uint32_t sizes[][2] = { { 37, 29 }, { 1, 1 }, { 3, 64 } };
            for (const auto &wh : sizes)
                for (int grey = 0; grey < 2; grey++) {
                    const uint32_t W = wh[0], H = wh[1];
                    std::vector<float> z((size_t)W * H);
                    std::vector<uint8_t> rgb(3 * (size_t)W * H), keep;
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
                    keep = rgb;
                    tr::ao_host(W, H, z.data(), rgb.data(), radius, rings, grey != 0, 1.0f, 20.0f);
                    size_t changed = 0;
                    for (uint32_t y = 0; y < H; y++)
                        for (uint32_t x = 0; x < W; x++) {
                            const size_t c = 3 * ((size_t)(H - 1 - y) * W + x);
                            const bool same = memcmp(&rgb[c], &keep[c], 3) == 0;
                            if (!tr::ao_drawn(z[x + (size_t)y * W])) bad += !same;
                            changed += !same;
                        }
                    if (W > 1 && radius <= 8) bad += changed == 0;
                    // a flat field occludes nothing: plain shading keeps every byte
                    for (float &v : z) v = 42.0f;
                    rgb = keep;
                    tr::ao_host(W, H, z.data(), rgb.data(), radius, rings, false, 1.0f, 20.0f);
                    bad += rgb != keep;
                }
        }
    // a pixel at the foot of a step of 30 with one ring of radius 1: the samples (0, 1) -- three times: i = 15, 0, 1 --
    // and (1, 1) above it occlude, s = 1 each: coef = 1 - 4/16
    {
        const uint32_t W = 3, H = 3;
        std::vector<float> z = { 10, 10, 10, 10, 10, 10, 10, 40, 40 };   // row y = 2 (top): x = 1, 2 raised
        std::vector<uint8_t> rgb(27, 160);
        tr::ao_host(W, H, z.data(), rgb.data(), 1, 1, false, 1.0f, 20.0f);
        const uint8_t *c = &rgb[3 * ((H - 1 - 1) * W + 1)];               // pixel (1, 1)
        bad += c[0] != 120 || c[1] != 120 || c[2] != 120;                 // 160 * (1 - 4/16) = 120
        printf("centre pixel %u (120 expected)\n", c[0]);
    }
    printf("%d mismatches\n", bad);
    return bad ? 1 : 0;
}
