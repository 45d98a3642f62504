// projector_host_check.cpp -- the host half of the projector (projector_host -- the body of tr_projector_host -- and the
// inline functions k_projector calls, tr_projector.h) against a plain re-derivation: every f32 step through a volatile
// float, the integer steps in 64 bits with true divisions, texels fetched one byte at a time.  Random small frames,
// images of 1 x 1 up to 9 x 7 in both channel counts at padded strides, matrices with a perspective row (w of both signs,
// zero and huge), the special depths (NaN, +-inf, f32::MIN, denormals), occluders with undrawn and NaN texels, every
// mode, hard and SOFT, in place and out of place -- over heap blocks EXACTLY as large as the function may touch: the image
// ends with its last pixel, the occluder with its last float, so a byte read outside them (the texel behind the closed
// upper edge) is an error under the sanitizer.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/projector_host_check.cpp -o projector_host_check && ./projector_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tr_projector.h"

using namespace tr;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}
static float unit() { return (float)(rnd() >> 8) / 16777216.0f; }              // [0, 1)
static float range(float lo, float hi) { return lo + (hi - lo) * unit(); }

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

// One pixel by the words of the header.  Returns false where the pixel keeps its colour.
static bool pixel64(const ProjectorRule &q, const uint8_t *image, const float *occ, int x, int y, float z, const uint8_t d[3], uint8_t o[3])
{
    if (f32_bits(z) == 0xFF7FFFFFu) return false;
    volatile float c[4];
    for (int i = 0; i < 4; i++) {
        volatile float t0 = q.m[i] * (float)x, t1 = q.m[4 + i] * (float)y, t2 = q.m[8 + i] * z;
        volatile float s0 = t0 + t1;
        volatile float s1 = s0 + t2;
        c[i] = s1 + q.m[12 + i];
    }
    const float w = c[3];
    if (!(w > 0.0f) || isinf(w)) return false;
    volatile float r = 1.0f / w;
    volatile float u = c[0] * r, v = c[1] * r, zp = c[2] * r;
    if (!(u >= 0.0f && u <= (float)(q.pw - 1u) && v >= 0.0f && v <= (float)(q.ph - 1u))) return false;
    const int64_t su = (int64_t)floor((double)u * 256.0), sv = (int64_t)floor((double)v * 256.0);
    const int64_t ix = su >> 8, ax = su & 255, iy = sv >> 8, ay = sv & 255;
    const int64_t wt[4] = { (256 - ax) * (256 - ay), ax * (256 - ay), (256 - ax) * ay, ax * ay };
    int64_t sum[4] = { 0, 0, 0, 0 }, lit = 0;
    volatile float zt = zp + q.depth_bias;
    for (int t = 0; t < 4; t++) {
        if (wt[t] == 0) continue;
        const int64_t i = ix + (t & 1), j = iy + (t >> 1);
        const uint8_t *p = image + ((int64_t)q.ph - 1 - j) * (int64_t)q.stride + i * (int64_t)q.bpp;
        for (int ch = 0; ch < 4; ch++) sum[ch] += wt[t] * (ch < (int)q.bpp ? (int64_t)p[ch] : 255);
        if (occ && !(zt < occ[j * (int64_t)q.pw + i])) lit += wt[t];
    }
    int64_t f = 256;
    if (q.flags & PROJECTOR_OCCLUDE) {
        if (q.flags & PROJECTOR_SOFT) f = (lit + 128) >> 8;
        else f = !(zt < occ[(iy + (ay >= 128)) * (int64_t)q.pw + ix + (ax >= 128)]) ? 256 : 0;
    }
    const int64_t alpha = (sum[3] + 32768) >> 16, a = (alpha * (int64_t)q.opacity * f + 128) >> 8;
    for (int ch = 0; ch < 3; ch++) {
        const int64_t s = (sum[ch] + 32768) >> 16;
        o[ch] = (uint8_t)((blend64(q.mode, s, d[ch]) * a + (int64_t)d[ch] * (65280 - a) + 32640) / 65280);
    }
    return true;
}

static float special_depth(uint32_t k)
{
    switch (k % 8u) {
    case 0: return bits_f32(0xFF7FFFFFu);  // not drawn
    case 1: return NAN;
    case 2: return INFINITY;
    case 3: return -INFINITY;
    case 4: return bits_f32(1u);           // a denormal
    case 5: return -0.0f;
    default: return range(10.0f, 90.0f);
    }
}

int main()
{
    long n_px = 0, n_hit = 0, n_edge = 0, n_shadow = 0, n_part = 0;
    for (int k = 0; k < 4000; k++) {
        const uint32_t W = 1u + rnd() % 12u, H = 1u + rnd() % 7u;
        ProjectorRule q = {};
        q.pw = 1u + rnd() % 9u, q.ph = 1u + rnd() % 7u, q.bpp = 3u + (rnd() & 1u);
        q.stride = q.pw * q.bpp + rnd() % 6u;
        q.mode = rnd() % LAYER_MODES, q.opacity = (k % 5 == 0) ? 256u : rnd() % 257u;
        q.flags = (uint32_t[]){ 0u, PROJECTOR_OCCLUDE, PROJECTOR_OCCLUDE | PROJECTOR_SOFT }[rnd() % 3u];
        q.depth_bias = (k % 3 == 0) ? 0.0f : range(-4.0f, 4.0f);
        const float sx = (float)q.pw / (float)W, sy = (float)q.ph / (float)H;
        const float m[16] = { range(0.5f, 1.5f) * sx, range(-0.2f, 0.2f), range(-0.1f, 0.1f), range(-0.05f, 0.05f),
                              range(-0.2f, 0.2f), range(0.5f, 1.5f) * sy, range(-0.1f, 0.1f), range(-0.05f, 0.05f),
                              range(-0.02f, 0.02f), range(-0.02f, 0.02f), range(0.5f, 1.5f), range(-0.01f, 0.01f),
                              range(-1.0f, 1.0f), range(-1.0f, 1.0f), range(-5.0f, 5.0f), range(0.2f, 1.5f) };
        memcpy(q.m, m, sizeof m);
        if (k % 7 == 0) {  // an exact scale: the closed upper edge u == pw - 1, v == ph - 1 is reached
            memset(q.m, 0, sizeof q.m);
            q.m[0] = W > 1u ? (float)(q.pw - 1u) / (float)(W - 1u) : 0.0f, q.m[5] = H > 1u ? (float)(q.ph - 1u) / (float)(H - 1u) : 0.0f;
            q.m[10] = 1.0f, q.m[15] = 1.0f;
            if (W == 1u) q.m[12] = (float)(q.pw - 1u);
            if (H == 1u) q.m[13] = (float)(q.ph - 1u);
        }
        if (k % 11 == 0) q.m[15] = 0.0f, q.m[3] = 0.0f, q.m[7] = 0.0f, q.m[11] = 0.0f;  // w == 0 everywhere
        if (k % 13 == 0) q.m[15] = 3.0e38f, q.m[11] = 3.0e38f;                            // w overflows
        // heap blocks exactly as large as the rule may touch
        const size_t n = (size_t)W * H, image_bytes = (size_t)projector_image_bytes(q), occ_n = (size_t)q.pw * q.ph;
        uint8_t *rgb = (uint8_t *)malloc(n * 3), *out = (uint8_t *)malloc(n * 3), *want = (uint8_t *)malloc(n * 3), *image = (uint8_t *)malloc(image_bytes);
        float *z = (float *)malloc(n * sizeof(float)), *occ = (float *)malloc(occ_n * sizeof(float));
        for (size_t i = 0; i < n * 3; i++) rgb[i] = (uint8_t)rnd();
        for (size_t i = 0; i < image_bytes; i++) image[i] = (uint8_t)rnd();
        for (size_t i = 0; i < n; i++) z[i] = (k % 4 == 0) ? special_depth(rnd()) : ((rnd() % 5u == 0u) ? bits_f32(0xFF7FFFFFu) : range(10.0f, 90.0f));
        for (size_t i = 0; i < occ_n; i++) {
            const uint32_t pick = rnd() % 6u;
            occ[i] = pick == 0u ? bits_f32(0xFF7FFFFFu) : pick == 1u ? NAN : range(0.0f, 120.0f);
        }
        const float *occ_arg = (q.flags & PROJECTOR_OCCLUDE) ? occ : nullptr;
        memcpy(want, rgb, n * 3);
        for (uint32_t r = 0; r < H; r++)
            for (uint32_t x = 0; x < W; x++) {
                const uint32_t y = H - 1u - r;
                uint8_t o[3];
                const uint8_t *d = rgb + ((size_t)r * W + x) * 3;
                n_px++;
                if (!pixel64(q, image, occ_arg, (int)x, (int)y, z[x + (size_t)y * W], d, o)) continue;
                memcpy(want + ((size_t)r * W + x) * 3, o, 3);
                n_hit++;
                ProjectorAt h;
                if (projector_at(q, (int32_t)x, (int32_t)y, z[x + (size_t)y * W], h)) {
                    if (h.ix == (int32_t)q.pw - 1 || h.iy == (int32_t)q.ph - 1) n_edge++;
                    if (occ_arg) {
                        const ProjectorHostZ zo = { occ, q.pw };
                        const uint32_t f = projector_light(q, h, zo);
                        n_shadow += f == 0u, n_part += f > 0u && f < 256u;
                    }
                }
            }
        memset(out, 0xAA, n * 3);
        projector_host(W, H, rgb, z, q, image, occ_arg, out);
        if (memcmp(out, want, n * 3) != 0) return fail("projector_host, out of place", k, (long)W, (long)H);
        memcpy(out, rgb, n * 3);
        projector_host(W, H, out, z, q, image, occ_arg, out);
        if (memcmp(out, want, n * 3) != 0) return fail("projector_host, in place", k, (long)W, (long)H);
        free(rgb), free(out), free(want), free(image), free(z), free(occ);
    }
    if (n_hit < n_px / 20 || n_px - n_hit < n_px / 20 || n_edge < 100 || n_shadow < 100 || n_part < 100)
        return fail("the cases do not reach what they are for", n_hit, n_edge, n_shadow + n_part);
    printf("projector_host_check: %ld pixels, %ld covered, %ld on the closed upper edge, %ld shadowed, %ld partly lit: ok\n", n_px, n_hit, n_edge, n_shadow,
           n_part);
    return 0;
}
