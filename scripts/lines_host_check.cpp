// lines_host_check.cpp -- the host half of the lines stage (lines_host -- the body of tr_lines_host --, lines_bin --
// tr_scene_set_lines' binning -- and the inline functions k_lines calls, tr_lines.h) against naive code: the floor
// division against the truncating 64-bit '/' with its remainder's sign handled, over operands up to both bounds;
// lines_host against a naive rule that walks every step of every segment with that division, keeps the winner as a
// plain comparison of (key, index) and blends with true divisions, over small random frames and tables whose segments
// are short, long, axis-parallel, exact diagonals, single pixels, far outside and at +-2^20, every width, with and
// without the test and under PAINTER, in place and out of place; and the bins against the brute force "which tiles hold a
// pixel of the segment at width 15", with the lists ascending and `tiles` the non-empty ones.  Everything runs over heap
// blocks exactly as large as the functions may touch: a byte read or written outside them is an error under the
// sanitizer.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/lines_host_check.cpp -o lines_host_check && ./lines_host_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <vector>

#include "tr_lines.h"

using namespace tr;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}
static int32_t between(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

static int fail(const char *what, long a = 0, long b = 0, long c = 0)
{
    printf("FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

static int64_t floor64(int64_t num, int64_t den)
{
    int64_t q = num / den;
    if (num % den != 0 && ((num < 0) != (den < 0))) q -= 1;
    return q;
}

static Line random_line(int32_t W, int32_t H, uint32_t i)
{
    const int32_t L = LINES_COORD_MAX;
    Line l;
    l.x0 = between(-4, W + 3), l.y0 = between(-4, H + 3);
    switch (i % 7u) {
    case 0: l.x1 = l.x0 + between(-12, 12), l.y1 = l.y0 + between(-12, 12); break;
    case 1: l.x1 = between(-4, W + 3), l.y1 = between(-4, H + 3); break;
    case 2:
        if (rnd() & 1u) l.x1 = between(-4, W + 3), l.y1 = l.y0;
        else l.x1 = l.x0, l.y1 = between(-4, H + 3);
        break;
    case 3: {
        const int32_t d = between(-W - H, W + H);
        l.x1 = l.x0 + d, l.y1 = l.y0 + ((rnd() & 1u) ? d : -d);
        break;
    }
    case 4: l.x1 = l.x0, l.y1 = l.y0; break;
    case 5: l.x1 = l.x0 + between(-5000, 5000), l.y1 = l.y0 + between(-5000, 5000); break;
    default:
        l.x1 = (rnd() & 1u) ? L : -L, l.y1 = (rnd() & 1u) ? L : -L;
        if (rnd() & 1u) l.x0 = -l.x1, l.y0 = (rnd() & 1u) ? -l.y1 : between(-4, H + 3);
        break;
    }
    l.z0 = (float)(rnd() % 10000u) / 100.0f, l.z1 = (i % 3u == 0u) ? l.z0 : (float)(rnd() % 10000u) / 100.0f;
    if (i % 3u == 0u) l.z0 = l.z1 = 25.0f * (float)(1u + (i / 3u) % 3u);
    l.rgba = rnd();
    if (rnd() & 1u) l.rgba |= 0xFF000000u;
    l.reserved = 0u;
    return l;
}

// The rule, naively: every step of every segment, the frame test a step, (key, index) compared as a pair.
static void naive(int32_t W, int32_t H, const uint8_t *rgb, const float *z, const LinesRule &q, uint32_t n, const Line *lines, uint8_t *out)
{
    std::vector<uint32_t> key((size_t)W * H, 0u), who((size_t)W * H, 0u);  // who: index + 1
    for (uint32_t i = 0; i < n; i++) {
        Line l = lines[i];
        const int64_t dx = (int64_t)l.x1 - l.x0, dy = (int64_t)l.y1 - l.y0;
        const bool xm = llabs(dx) >= llabs(dy);
        int64_t a0 = xm ? l.x0 : l.y0, a1 = xm ? l.x1 : l.y1, b0 = xm ? l.y0 : l.x0, b1 = xm ? l.y1 : l.x1;
        float z0 = l.z0, z1 = l.z1;
        if (a1 < a0) std::swap(a0, a1), std::swap(b0, b1), std::swap(z0, z1);
        const int64_t nn = a1 - a0, db = b1 - b0;
        // (walking 2^21 steps of a segment at the limit is too slow here: only the steps near the frame)
        const int64_t k_first = std::max<int64_t>(0, -a0 - 2), k_last = std::min<int64_t>(nn, (xm ? W : H) + 1 - a0);
        for (int64_t k = k_first; k <= k_last; k++) {
            const int64_t bc = nn ? b0 + floor64(2 * k * db + nn, 2 * nn) : b0;
            volatile float t = nn ? (float)k / (float)nn : 0.0f;
            volatile float dz = z1 - z0;
            volatile float m = dz * t;
            volatile float zz = z0 + m;
            volatile float zl = zz + q.bias;
            for (int64_t o = -(((int64_t)q.width - 1) / 2); o <= (int64_t)q.width / 2; o++) {
                const int64_t x = xm ? a0 + k : bc + o, y = xm ? bc + o : a0 + k;
                if (x < 0 || x >= W || y < 0 || y >= H) continue;
                const size_t at = (size_t)(x + y * W);
                if ((q.flags & LINES_DEPTH_TEST) && zl <= z[at]) continue;
                const float zf = zl;
                uint32_t bits;
                memcpy(&bits, &zf, 4);
                const uint32_t ky = (q.flags & LINES_PAINTER) ? 0u : ((bits >> 31) ? ~bits : bits ^ 0x80000000u);
                if (who[at] == 0u || ky > key[at] || (ky == key[at] && i + 1u > who[at])) key[at] = ky, who[at] = i + 1u;
            }
        }
    }
    if (out != rgb) memmove(out, rgb, (size_t)W * H * 3u);
    for (int32_t y = 0; y < H; y++)
        for (int32_t x = 0; x < W; x++) {
            const uint32_t w = who[(size_t)(x + y * W)];
            if (!w) continue;
            uint8_t *o = out + ((size_t)(H - 1 - y) * W + x) * 3u;
            const uint32_t c = lines[w - 1u].rgba;
            const int64_t a = (int64_t)(c >> 24) * q.opacity;
            for (int ch = 0; ch < 3; ch++) o[ch] = (uint8_t)((((c >> (8 * ch)) & 0xFFu) * a + o[ch] * (65280 - a) + 32640) / 65280);
        }
}

int main()
{
    long n_div = 0, n_frames = 0, n_binned = 0;
    // the floor division: random operands up to both bounds, and the neighbourhood of every multiple
    for (int it = 0; it < 400000; it++) {
        const int32_t den = it % 5 == 0 ? (1 << 22) - (int32_t)(rnd() % 64u) : 1 + (int32_t)(rnd() % (1u << 22));
        const int64_t span = (int64_t)den << 22;  // (the rule's quotients stay within +-2^22)
        int64_t num = (int64_t)(((uint64_t)rnd() << 32 | rnd()) % (uint64_t)(2 * span + 1)) - span;
        if (it % 3 == 0) num = (num / den) * den + (int64_t)between(-2, 2);
        if (lines_floor_div(num, den) != floor64(num, den)) return fail("lines_floor_div", (long)num, den);
        n_div++;
    }
    for (int it = 0; it < 160; it++) {
        const int32_t W = it % 4 == 0 ? 128 + between(1, 140) : between(1, 70), H = it % 5 == 0 ? between(17, 40) : between(1, 24);
        const uint32_t n = it % 9 == 0 ? 0u : (uint32_t)between(1, 80);
        // heap blocks exactly as large as the rule may touch
        uint8_t *rgb = (uint8_t *)malloc((size_t)W * H * 3), *out = (uint8_t *)malloc((size_t)W * H * 3), *ref = (uint8_t *)malloc((size_t)W * H * 3);
        float *z = (float *)malloc((size_t)W * H * sizeof(float));
        Line *lines = (Line *)malloc(n ? n * sizeof(Line) : 1);
        for (size_t k = 0; k < (size_t)W * H * 3; k++) rgb[k] = (uint8_t)rnd();
        for (size_t k = 0; k < (size_t)W * H; k++) {
            const uint32_t r = rnd() % 8u;
            z[k] = r < 3u ? bits_f32(TR_F32_MIN_BITS) : r == 3u && k % 11 == 0 ? NAN : (float)(rnd() % 10000u) / 100.0f;
        }
        for (uint32_t i = 0; i < n; i++) {
            lines[i] = random_line(W, H, i + (uint32_t)it);
            if (lines_refusal(lines[i])) return fail("a generated segment is refused", it, i);
        }
        LinesRule q;
        q.width = 1u + (uint32_t)it % 15u;
        q.opacity = it % 6 == 0 ? 256u : rnd() % 257u;
        q.flags = (it % 3 ? LINES_DEPTH_TEST : 0u) | (it % 7 == 3 ? LINES_PAINTER : 0u);
        q.bias = it % 4 == 1 ? 0.75f : it % 4 == 2 ? -1.5f : 0.0f;
        naive(W, H, rgb, z, q, n, lines, ref);
        lines_host((uint32_t)W, (uint32_t)H, rgb, (q.flags & LINES_DEPTH_TEST) ? z : nullptr, q, n, lines, out);
        if (memcmp(out, ref, (size_t)W * H * 3)) return fail("lines_host out of place", it, W, H);
        memcpy(out, rgb, (size_t)W * H * 3);
        lines_host((uint32_t)W, (uint32_t)H, out, (q.flags & LINES_DEPTH_TEST) ? z : nullptr, q, n, lines, out);
        if (memcmp(out, ref, (size_t)W * H * 3)) return fail("lines_host in place", it, W, H);
        n_frames++;
        // the bins: brute force over the pixels at width 15, with the naive division
        std::vector<uint64_t> offsets;
        std::vector<uint32_t> entries, tiles;
        lines_bin((uint32_t)W, (uint32_t)H, n, lines, offsets, entries, tiles);
        const int32_t ntx = (W + TILE_W - 1) / TILE_W, nty = (H + TILE_H - 1) / TILE_H;
        if ((int64_t)offsets.size() != (int64_t)ntx * nty + 1 || offsets[0] != 0u || offsets.back() != entries.size()) return fail("the offsets' ends", it);
        std::vector<std::set<uint32_t>> want((size_t)ntx * nty);
        for (uint32_t i = 0; i < n; i++) {
            const LineGeom g = lines_geom(lines[i]);
            const int64_t k_first = std::max<int64_t>(0, -(int64_t)g.a0), k_last = std::min<int64_t>(g.n, (g.xmajor ? W : H) - 1 - (int64_t)g.a0);
            for (int64_t k = k_first; k <= k_last; k++) {
                const int64_t bc = g.n ? g.b0 + floor64(2 * k * g.db + g.n, 2 * (int64_t)g.n) : g.b0;
                for (int64_t o = -7; o <= 7; o++) {
                    const int64_t x = g.xmajor ? g.a0 + k : bc + o, y = g.xmajor ? bc + o : g.a0 + k;
                    if (x >= 0 && x < W && y >= 0 && y < H) want[(size_t)((y / TILE_H) * ntx + x / TILE_W)].insert(i);
                }
            }
        }
        size_t t_at = 0;
        for (size_t t = 0; t < want.size(); t++) {
            const std::vector<uint32_t> got(entries.begin() + (ptrdiff_t)offsets[t], entries.begin() + (ptrdiff_t)offsets[t + 1]);
            if (got != std::vector<uint32_t>(want[t].begin(), want[t].end())) return fail("a tile's list", it, (long)t, (long)got.size());
            if (!got.empty() && (t_at >= tiles.size() || tiles[t_at++] != t)) return fail("the list of non-empty tiles", it, (long)t);
        }
        if (t_at != tiles.size()) return fail("the list of non-empty tiles is too long", it);
        n_binned++;
        free(rgb), free(out), free(ref), free(z), free(lines);
    }
    // a diagonal across a wide frame lands in O(tiles crossed) lists
    {
        Line l = { 0, 0, 1.0f, 1023, 127, 2.0f, 0xFFFFFFFFu, 0u };
        std::vector<uint64_t> offsets;
        std::vector<uint32_t> entries, tiles;
        lines_bin(1024u, 128u, 1u, &l, offsets, entries, tiles);
        if (entries.size() > 32u || entries.size() < 8u) return fail("the diagonal's entries", (long)entries.size());
    }
    printf("lines: %ld floor divisions, %ld frames, %ld binned tables, 0 mismatches\n", n_div, n_frames, n_binned);
    return 0;
}
