// layer_host_check.cpp -- the host half of the layer stage (layer_host -- the body of tr_layer_host -- and the inline
// functions k_layer calls, tr_layer.h) against a naive loop in 64-bit integers with true divisions, over small random
// frames and layers of both formats, every mode, the flags, opacities 0 .. 256, rectangles that hang over every edge or
// miss the frame and strides larger than the row; layer_fetch -- the aligned words and funnel shifts k_layer loads a
// unit's layer pixels with -- for every byte alignment of the block, every partly covered unit and both ends of the
// block; and both division identities over their whole ranges.  A stand-alone program over heap blocks exactly as large
// as the functions may touch: a word loaded outside the layer's bytes is an error under the sanitizer.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/layer_host_check.cpp -o layer_host_check && ./layer_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tr_layer.h"

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

// The rule's text over a block of exactly 3 W H bytes, in int64.
static void naive(int64_t W, int64_t H, const uint8_t *rgb, const float *z, const LayerRule &q, const uint8_t *image, uint8_t *out)
{
    const int64_t bpp = q.format == LAYER_RGBA8 ? 4 : 3;
    memcpy(out, rgb, (size_t)(W * H * 3));
    for (int64_t r = 0; r < H; r++)
        for (int64_t x = 0; x < W; x++) {
            const int64_t lx = x - q.x, ly = r - q.y;
            if (lx < 0 || ly < 0 || lx >= (int64_t)q.width || ly >= (int64_t)q.height) continue;
            const uint8_t *s = image + ly * (int64_t)q.stride + lx * bpp;
            int64_t a = (bpp == 4 ? s[3] : 255) * (int64_t)q.opacity;
            if ((q.flags & LAYER_KEY) && s[0] == (q.key & 0xFF) && s[1] == ((q.key >> 8) & 0xFF) && s[2] == ((q.key >> 16) & 0xFF)) a = 0;
            if (q.flags & (LAYER_WHERE_DRAWN | LAYER_WHERE_UNDRAWN)) {
                uint32_t zb;
                memcpy(&zb, &z[x + (H - 1 - r) * W], 4);
                const bool drawn = zb != 0xFF7FFFFFu;
                if ((q.flags & LAYER_WHERE_DRAWN) ? !drawn : drawn) a = 0;
            }
            for (int c = 0; c < 3; c++) {
                const int64_t d = rgb[(r * W + x) * 3 + c];
                out[(r * W + x) * 3 + c] = (uint8_t)((blend64(q.mode, s[c], d) * a + d * (65280 - a) + 32640) / 65280);
            }
        }
}

int main()
{
    // the divisions, over their whole ranges
    for (uint32_t n = 0; n <= 255u * 65280u + 32640u; n++)
        if (layer_div65280(n) != n / 65280u) return fail("layer_div65280", (long)n);
    for (uint32_t x = 0; x < 65536u; x++)
        if (layer_div255(x) != x / 255u) return fail("layer_div255", (long)x);

    // layer_host against the naive loop
    long frames = 0, bytes = 0;
    const uint32_t opacities[] = { 0u, 1u, 128u, 255u, 256u };
    const float z_min = -3.40282347e+38f;
    for (int round = 0; round < 1200; round++) {
        const int64_t W = 1 + rnd() % 23, H = 1 + rnd() % 17;
        LayerRule q;
        q.mode = (uint32_t)round % LAYER_MODES;
        q.format = (round / 7) % 2 ? LAYER_RGBA8 : LAYER_RGB8;
        const uint32_t where = (round / 14) % 3;
        q.flags = (where == 1 ? LAYER_WHERE_DRAWN : where == 2 ? LAYER_WHERE_UNDRAWN : 0u) | (rnd() % 3 == 0 ? LAYER_KEY : 0u);
        q.opacity = opacities[rnd() % 5];
        q.width = 1 + rnd() % 19, q.height = 1 + rnd() % 13;
        // mostly overlapping the frame, over any edge; sometimes far away
        q.x = (int32_t)(rnd() % (uint32_t)(W + q.width + 4)) - (int32_t)q.width - 2;
        q.y = (int32_t)(rnd() % (uint32_t)(H + q.height + 4)) - (int32_t)q.height - 2;
        if (round % 97 == 0) q.x = round % 2 ? INT32_MIN : INT32_MAX, q.y = round % 3 ? INT32_MAX : INT32_MIN;
        const uint32_t bpp = layer_bpp(q.format);
        q.stride = q.width * bpp + (rnd() % 2 ? rnd() % 9 : 0u);
        q.key = rnd() & 0x010101u;  // (few colours, so that it is met)
        const size_t n_img = (size_t)layer_block_bytes(q.width, q.height, q.stride, q.format), n_fb = (size_t)(W * H * 3);
        uint8_t *image = (uint8_t *)malloc(n_img), *rgb = (uint8_t *)malloc(n_fb), *want = (uint8_t *)malloc(n_fb), *got = (uint8_t *)malloc(n_fb);
        float *z = (float *)malloc((size_t)(W * H) * 4);
        for (size_t i = 0; i < n_img; i++) image[i] = (uint8_t)(rnd() % 5 == 0 ? rnd() & 1u : rnd());
        if (bpp == 4)
            for (size_t i = 3; i < n_img; i += 4)
                if (rnd() % 3 == 0) image[i] = rnd() % 2 ? 255 : 0;
        for (size_t i = 0; i < n_fb; i++) rgb[i] = (uint8_t)rnd();
        for (int64_t i = 0; i < W * H; i++) z[i] = rnd() % 2 ? z_min : (float)(rnd() % 1000) * 0.01f;
        const float *zz = where ? z : nullptr;
        naive(W, H, rgb, z, q, image, want);
        layer_host((uint32_t)W, (uint32_t)H, rgb, zz, q, image, got);
        if (memcmp(got, want, n_fb) != 0) return fail("layer_host out of place", round, (long)q.mode, (long)q.flags);
        memcpy(got, rgb, n_fb);
        layer_host((uint32_t)W, (uint32_t)H, got, zz, q, image, got);
        if (memcmp(got, want, n_fb) != 0) return fail("layer_host in place", round, (long)q.mode, (long)q.flags);
        frames++, bytes += (long)n_fb;
        free(image), free(rgb), free(want), free(got), free(z);
    }

    // layer_fetch: a block of `total` bytes at every alignment (malloc returns 16-byte aligned memory; the block ends
    // with the allocation), a unit of four pixels at every pixel offset from three pixels before the block to its end,
    // every covered range [j0, j1) of it that lies inside the block
    long fetches = 0;
    for (int bpp = 3; bpp <= 4; bpp++)
        for (int n_px = 1; n_px <= 33; n_px++)
            for (int lead = 0; lead < 4; lead++) {
                const int64_t total = (int64_t)n_px * bpp;
                uint8_t *mem = (uint8_t *)malloc((size_t)(lead + total));
                uint8_t *image = mem + lead;
                for (int64_t i = 0; i < lead + total; i++) mem[i] = (uint8_t)rnd();
                for (int first = -3; first < n_px; first++)
                    for (int j0 = 0; j0 < 4; j0++)
                        for (int j1 = j0 + 1; j1 <= 4; j1++) {
                            if (first + j0 < 0 || first + j1 > n_px) continue;
                            const int64_t u0 = (int64_t)first * bpp;
                            uint32_t px[4] = { 0u, 0u, 0u, 0u };
                            if (bpp == 3) layer_fetch<3>(image, total, u0, u0 + j0 * 3, u0 + j1 * 3, px);
                            else layer_fetch<4>(image, total, u0, u0 + j0 * 4, u0 + j1 * 4, px);
                            for (int i = j0; i < j1; i++) {
                                const uint8_t *s = image + u0 + (int64_t)i * bpp;
                                const uint32_t want = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((bpp == 4 ? (uint32_t)s[3] : 255u) << 24);
                                if (px[i] != want) return fail("layer_fetch", bpp, first, i);
                            }
                            fetches++;
                        }
                free(mem);
            }

    // the facts
    for (uint32_t mode = 0; mode < LAYER_MODES; mode++)
        for (uint32_t s = 0; s < 256u; s += 5u)
            for (uint32_t d = 0; d < 256u; d += 3u) {
                const uint32_t sp = s | (s << 8) | (s << 16), dp = d | (d << 8) | (d << 16);
                if (layer_px_by(mode, sp, dp, 0u) != dp) return fail("coverage 0 leaves d", (long)mode, (long)s, (long)d);
                const uint32_t b = (uint32_t)blend64(mode, s, d);
                if (layer_px_by(mode, sp, dp, LAYER_FULL) != (b | (b << 8) | (b << 16))) return fail("full coverage gives b", (long)mode, (long)s, (long)d);
            }
    for (uint32_t d = 0; d < 256u; d++) {
        if (layer_blend<LAYER_MULTIPLY>(255u, d) != d || layer_blend<LAYER_ADD>(0u, d) != d || layer_blend<LAYER_DIFFERENCE>(d, d) != 0u)
            return fail("identities", (long)d);
    }
    printf("layer: %ld frames, %ld fetches, 0 mismatches (%ld bytes)\n", frames, fetches, bytes);
    return 0;
}
