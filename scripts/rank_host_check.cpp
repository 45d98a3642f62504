// rank_host_check.cpp -- the host half of the rank stage (rank_host -- the body of tr_rank_host --, the parameter check and
// the inline functions k_rank shares, tr_rank.h) against a naive gather and sort, over small random images, random
// footprints, ranks, ops and both edge modes, plus the copy, the constant-frame and the refusal facts, as a stand-alone
// program over heap blocks exactly as large as the function may touch.
// For the CPU only:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude
//       -Itiny_renderer_amd/csrc scripts/rank_host_check.cpp -o rank_host_check && ./rank_host_check
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "tr_rank.h"

using namespace tr;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 32);
}
static int32_t between(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }
static int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// The rule's text, one pixel and channel at a time: gather, sort, index.
static uint8_t naive(int64_t W, int64_t H, const uint8_t *rgb, int64_t x, int64_t y, int c, const RankParams &p)
{
    uint8_t v[RANK_MAX_TAPS];
    uint32_t n = 0;
    for (int64_t j = 0; j < p.kh; j++)
        for (int64_t i = 0; i < p.kw; i++) {
            if (((p.rows[j] >> i) & 1u) == 0u) continue;
            int64_t sx = x + i - p.kw / 2, sy = y + j - p.kh / 2;
            if (p.edge == RANK_CLAMP) sx = clampi(sx, 0, W - 1), sy = clampi(sy, 0, H - 1);
            v[n++] = sx < 0 || sx >= W || sy < 0 || sy >= H ? p.border[c] : rgb[(sy * W + sx) * 3 + c];
        }
    std::sort(v, v + n);
    const int64_t F = rgb[(y * W + x) * 3 + c], lo = v[p.rank], hi = v[p.op == RANK_VALUE ? p.rank : p.rank2];
    if (p.op == RANK_RANGE) return (uint8_t)(hi - lo);
    if (p.op == RANK_MID) return (uint8_t)((lo + hi + 1) >> 1);
    if (p.op == RANK_CLAMP_CENTRE) return (uint8_t)std::min(std::max(F, lo), hi);
    return (uint8_t)lo;
}

static bool refused(const RankParams &p, const char *why)
{
    const char *got = rank_refusal(p);
    return got != nullptr && strcmp(got, why) == 0;
}

int main()
{
    int cases = 0;
    for (int round = 0; round < 600; round++) {
        RankParams p;
        memset(&p, 0, sizeof p);
        p.struct_size = sizeof p;
        p.kw = 2u * (rnd() % 8u) + 1u, p.kh = 2u * (rnd() % 8u) + 1u;
        const uint32_t density = rnd() % 4u;  // 0: every tap
        for (uint32_t j = 0; j < p.kh; j++)
            for (uint32_t i = 0; i < p.kw; i++)
                if (density == 0u || rnd() % (density + 1u) == 0u) p.rows[j] |= (uint16_t)(1u << i);
        if (rank_taps(p) == 0u) p.rows[rnd() % p.kh] = (uint16_t)(1u << (rnd() % p.kw));
        const uint32_t n = rank_taps(p);
        p.op = rnd() % 4u;
        const uint32_t a = rnd() % 3u == 0u ? (rnd() % 2u ? 0u : n - 1u) : rnd() % n, b = rnd() % 3u == 0u ? (rnd() % 2u ? 0u : n - 1u) : rnd() % n;
        p.rank = p.op == RANK_VALUE ? a : std::min(a, b), p.rank2 = p.op == RANK_VALUE ? 0u : std::max(a, b);
        p.edge = rnd() % 2u;
        p.border[0] = (uint8_t)rnd(), p.border[1] = (uint8_t)rnd(), p.border[2] = (uint8_t)rnd();
        if (rank_refusal(p) != nullptr) { fprintf(stderr, "round %d: refused: %s\n", round, rank_refusal(p)); return 1; }
        const RankRule q = rank_rule(p);
        if (q.n != n) return 1;
        const int64_t W = between(1, 40), H = between(1, 24);
        uint8_t *rgb = (uint8_t *)malloc((size_t)(W * H * 3)), *out = (uint8_t *)malloc((size_t)(W * H * 3));
        const uint32_t fill = rnd() % 3u;
        for (int64_t i = 0; i < W * H * 3; i++) rgb[i] = fill == 0u ? (uint8_t)rnd() : fill == 1u ? 255 : (uint8_t)(rnd() % 2u * 255u);
        rank_host((uint32_t)W, (uint32_t)H, rgb, out, q);
        for (int64_t y = 0; y < H; y++)
            for (int64_t x = 0; x < W; x++)
                for (int c = 0; c < 3; c++)
                    if (out[(y * W + x) * 3 + c] != naive(W, H, rgb, x, y, c, p)) {
                        fprintf(stderr, "round %d: (%lld, %lld)[%d] differs\n", round, (long long)x, (long long)y, c);
                        return 1;
                    }
        // the facts: one centre tap is a copy
        RankParams one;
        memset(&one, 0, sizeof one);
        one.struct_size = sizeof one, one.kw = p.kw, one.kh = p.kh, one.rows[p.kh / 2u] = (uint16_t)(1u << (p.kw / 2u)), one.edge = p.edge;
        rank_host((uint32_t)W, (uint32_t)H, rgb, out, rank_rule(one));
        if (memcmp(rgb, out, (size_t)(W * H * 3)) != 0) { fprintf(stderr, "round %d: one centre tap is no copy\n", round); return 1; }
        // a constant frame under CLAMP stays, and its RANGE is 0
        RankParams flat = p;
        flat.edge = RANK_CLAMP;
        const uint32_t c = rnd() % 256u, expect = p.op == RANK_RANGE ? 0u : c;
        memset(rgb, (int)c, (size_t)(W * H * 3));
        rank_host((uint32_t)W, (uint32_t)H, rgb, out, rank_rule(flat));
        for (int64_t i = 0; i < W * H * 3; i++)
            if (out[i] != expect) { fprintf(stderr, "round %d: a constant frame\n", round); return 1; }
        free(rgb), free(out);
        cases++;
    }
    // the refusals, each with its text
    RankParams ok;
    memset(&ok, 0, sizeof ok);
    ok.struct_size = sizeof ok, ok.kw = ok.kh = 3u, ok.rows[0] = ok.rows[1] = ok.rows[2] = 7u, ok.rank = 4u;
    if (rank_refusal(ok) != nullptr) return 1;
    RankParams w = ok;
    w.struct_size = 60u;
    if (!refused(w, ": struct_size is not sizeof(tr_rank_params)")) return 1;
    w = ok, w.kw = 4u;
    if (!refused(w, ": kw and kh must be odd and 1..15")) return 1;
    w = ok, w.kh = 17u;
    if (!refused(w, ": kw and kh must be odd and 1..15")) return 1;
    w = ok, w.rows[1] = 8u;
    if (!refused(w, ": footprint bits outside the kw x kh box")) return 1;
    w = ok, w.rows[14] = 1u;
    if (!refused(w, ": footprint bits outside the kw x kh box")) return 1;
    w = ok, w.rows[0] = w.rows[1] = w.rows[2] = 0u;
    if (!refused(w, ": the footprint is empty")) return 1;
    w = ok, w.op = 4u;
    if (!refused(w, ": op must be TR_RANK_VALUE, TR_RANK_RANGE, TR_RANK_MID or TR_RANK_CLAMP_CENTRE")) return 1;
    w = ok, w.edge = 2u;
    if (!refused(w, ": edge must be TR_RANK_BORDER or TR_RANK_CLAMP")) return 1;
    w = ok, w.pad = 1u;
    if (!refused(w, ": pad and pad2 must be 0")) return 1;
    w = ok, w.pad2 = 1u;
    if (!refused(w, ": pad and pad2 must be 0")) return 1;
    w = ok, w.rank = 9u;
    if (!refused(w, ": rank and rank2 must be below the number of taps")) return 1;
    w = ok, w.rank2 = 1u;
    if (!refused(w, ": rank2 must be 0 under TR_RANK_VALUE")) return 1;
    w = ok, w.op = RANK_MID, w.rank2 = 3u;
    if (!refused(w, ": rank must not exceed rank2")) return 1;
    if (rank_finish_px(RANK_RANGE, 0u, 0u, 0x123456u) != 0u || rank_finish_px(RANK_MID, 0u, 0u, 0xFFFFFFu) != 0u ||
        rank_finish_px(RANK_CLAMP_CENTRE, 0x010203u, 0x090807u, 0x00FF05u) != 0x010805u)
        return 1;
    printf("rank_host_check: %d cases equal the gather and sort\n", cases);
    return 0;
}
