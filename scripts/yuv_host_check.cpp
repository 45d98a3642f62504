// yuv_host_check.cpp -- the host half of the YUV output stage (yuv_host -- the body of tr_yuv_host -- and the inline
// functions k_yuv calls, tr_yuv.h) against a naive loop in 64-bit integers with the clamps written out and the
// coefficients computed again in double, over small random images of even and odd sides, all three layouts and all four
// tables, plus the grey, black and clamp facts, as a stand-alone program over heap blocks exactly as large as the
// function may touch.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/yuv_host_check.cpp -o yuv_host_check && ./yuv_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tr_yuv.h"

using namespace tr;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}

static int64_t clamp8(int64_t v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// The table of (matrix, range) from Kr and Kb in double: nearest integers, green adjusted to the row's sum.
struct Table {
    int64_t y[3], u[3], v[3], y0;
};
static Table derive(uint32_t matrix, uint32_t range)
{
    const double kr = matrix == YUV_BT601 ? 0.299 : 0.2126, kb = matrix == YUV_BT601 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
    const double sy = range == YUV_FULL ? 1.0 : 219.0 / 255.0, sc = range == YUV_FULL ? 1.0 : 224.0 / 255.0;
    const double yr[3] = { kr * sy, kg * sy, kb * sy };
    const double ur[3] = { -kr / (2 * (1 - kb)) * sc, -kg / (2 * (1 - kb)) * sc, 0.5 * sc };
    const double vr[3] = { 0.5 * sc, -kg / (2 * (1 - kr)) * sc, -kb / (2 * (1 - kr)) * sc };
    Table t;
    for (int c = 0; c < 3; c++) t.y[c] = llround(yr[c] * 65536.0), t.u[c] = llround(ur[c] * 65536.0), t.v[c] = llround(vr[c] * 65536.0);
    t.y[1] = llround(sy * 65536.0) - t.y[0] - t.y[2];
    t.u[1] = -t.u[0] - t.u[2];
    t.v[1] = -t.v[0] - t.v[2];
    t.y0 = range == YUV_FULL ? 0 : 16;
    return t;
}

// The rule's text into a block of exactly yuv_bytes bytes, in int64.
static void naive(int64_t W, int64_t H, const uint8_t *rgb, const Table &t, uint32_t layout, uint8_t *out)
{
    const int64_t cw = (W + 1) / 2, ch = (H + 1) / 2, wh = W * H;
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            const uint8_t *p = rgb + (y * W + x) * 3;
            out[y * W + x] = (uint8_t)clamp8((t.y[0] * p[0] + t.y[1] * p[1] + t.y[2] * p[2] + (t.y0 << 16) + 32768) >> 16);
            if (layout == YUV_I444) {
                out[wh + y * W + x] = (uint8_t)clamp8((t.u[0] * p[0] + t.u[1] * p[1] + t.u[2] * p[2] + (128 << 16) + 32768) >> 16);
                out[2 * wh + y * W + x] = (uint8_t)clamp8((t.v[0] * p[0] + t.v[1] * p[1] + t.v[2] * p[2] + (128 << 16) + 32768) >> 16);
            }
        }
    if (layout == YUV_I444) return;
    for (int64_t j = 0; j < ch; j++)
        for (int64_t i = 0; i < cw; i++) {
            const int64_t x1 = 2 * i + 1 < W ? 2 * i + 1 : W - 1, y1 = 2 * j + 1 < H ? 2 * j + 1 : H - 1;
            int64_t s[3];
            for (int c = 0; c < 3; c++)
                s[c] = (int64_t)rgb[(2 * j * W + 2 * i) * 3 + c] + rgb[(2 * j * W + x1) * 3 + c] + rgb[(y1 * W + 2 * i) * 3 + c] + rgb[(y1 * W + x1) * 3 + c];
            const uint8_t u = (uint8_t)clamp8((t.u[0] * s[0] + t.u[1] * s[1] + t.u[2] * s[2] + (128 << 18) + (1 << 17)) >> 18);
            const uint8_t v = (uint8_t)clamp8((t.v[0] * s[0] + t.v[1] * s[1] + t.v[2] * s[2] + (128 << 18) + (1 << 17)) >> 18);
            if (layout == YUV_NV12) out[wh + 2 * (j * cw + i)] = u, out[wh + 2 * (j * cw + i) + 1] = v;
            else out[wh + j * cw + i] = u, out[wh + cw * ch + j * cw + i] = v;
        }
}

static int fail(const char *what, long a = 0, long b = 0, long c = 0)
{
    printf("FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

int main()
{
    long images = 0, bytes = 0;
    for (uint32_t matrix = 0; matrix < 2; matrix++)
        for (uint32_t range = 0; range < 2; range++) {
            const Table t = derive(matrix, range);
            YuvRule k = kYuvTables[matrix][range];
            for (int c = 0; c < 3; c++)
                if (k.y[c] != t.y[c] || k.u[c] != t.u[c] || k.v[c] != t.v[c]) return fail("a coefficient differs from the derived one", matrix, range, c);
            if (k.y0 != t.y0) return fail("y0", matrix, range);
            if (k.u[0] + k.u[1] + k.u[2] != 0 || k.v[0] + k.v[1] + k.v[2] != 0) return fail("a chroma row does not sum to 0", matrix, range);
            // the facts: greys, black, the clamp at the top, nothing negative
            for (int32_t v = 0; v < 256; v++) {
                if (range == YUV_FULL && yuv_luma(k, v, v, v) != (uint32_t)v) return fail("a grey's Y in full range", v);
                if (yuv_chroma1(k.u, v, v, v) != 128u || yuv_chroma1(k.v, v, v, v) != 128u) return fail("a grey's chroma (4:4:4)", v);
                if (yuv_chroma4(k.u, 4 * v, 4 * v, 4 * v) != 128u || yuv_chroma4(k.v, 4 * v, 4 * v, 4 * v) != 128u) return fail("a grey's chroma (4:2:0)", v);
            }
            if (yuv_luma(k, 0, 0, 0) != (uint32_t)k.y0) return fail("black's Y");
            const int64_t blue_u = (yuv_dot(k.u, 0, 0, 255) + (128 << 16) + 32768) >> 16, red_v = (yuv_dot(k.v, 255, 0, 0) + (128 << 16) + 32768) >> 16;
            const int64_t blue_u4 = (yuv_dot(k.u, 0, 0, 1020) + (128 << 18) + (1 << 17)) >> 18, red_v4 = (yuv_dot(k.v, 1020, 0, 0) + (128 << 18) + (1 << 17)) >> 18;
            const int64_t top = range == YUV_FULL ? 256 : 240;
            if (blue_u != top || red_v != top || blue_u4 != top || red_v4 != top) return fail("pure blue's U or pure red's V before the clamp", blue_u, red_v, blue_u4);
            if (yuv_chroma1(k.u, 0, 0, 255) != (uint32_t)(top > 255 ? 255 : top)) return fail("the clamp");
            for (uint32_t layout = 0; layout < 3; layout++) {
                k.layout = layout;
                for (int round = 0; round < 40; round++) {
                    const uint32_t W = round < 4 ? 1u + (uint32_t)(round & 1) : 1u + rnd() % 37u, H = round < 4 ? 1u + (uint32_t)(round >> 1) : 1u + rnd() % 21u;
                    const size_t n_in = (size_t)W * H * 3u, n_out = yuv_bytes(W, H, layout);
                    uint8_t *rgb = (uint8_t *)malloc(n_in), *got = (uint8_t *)malloc(n_out), *want = (uint8_t *)malloc(n_out);
                    if (!rgb || !got || !want) return fail("malloc");
                    // noise, with the extremes frequent enough for the clamp to act
                    for (size_t i = 0; i < n_in; i++) {
                        const uint32_t r = rnd();
                        rgb[i] = (r & 0x300u) == 0u ? 0u : (r & 0x300u) == 0x100u ? 255u : (uint8_t)r;
                    }
                    memset(got, 0xAA, n_out), memset(want, 0x55, n_out);
                    yuv_host(W, H, rgb, k, got);
                    naive(W, H, rgb, t, layout, want);
                    if (memcmp(got, want, n_out) != 0) return fail("yuv_host differs from the naive loop", W, H, layout);
                    size_t off = 0, total = 0;
                    uint32_t pw = 0, ph = 0, step = 0;
                    for (uint32_t plane = 0; plane < yuv_n_planes(layout); plane++) {
                        if (!yuv_plane(W, H, layout, plane, &off, &pw, &ph, &step) || off != total) return fail("yuv_plane", W, H, plane);
                        total += (size_t)pw * ph * step;
                    }
                    if (total != n_out || yuv_plane(W, H, layout, yuv_n_planes(layout), &off, &pw, &ph, &step)) return fail("the planes do not tile yuv_bytes", W, H, layout);
                    free(rgb), free(got), free(want);
                    images++, bytes += (long)n_out;
                }
            }
        }
    printf("yuv: %ld images, %ld bytes, 0 mismatches\n", images, bytes);
    return 0;
}
