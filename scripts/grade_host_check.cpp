// grade_host_check.cpp -- the host half of colour grading (tr_grade.h: grade_host -- the body of tr_grade_host -- and the
// inline functions k_grade calls) as a stand-alone program, for a run under the host sanitizers.  Needs no GPU and does
// not load the library:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Itiny_renderer_amd/csrc scripts/grade_host_check.cpp -o grade_host_check
//   ./grade_host_check
// It grades colours held in arrays exactly as large as the function may touch, through tables of exactly 3 * N^3 bytes,
// against a second formulation of the rule written from its words: the six-case comparison chain of tetrahedral
// interpolation instead of a sort, in 64-bit integers with `/` and `%`.  N = 2, 3, 17, 25, 26 and 33; random tables;
// random colours, all 256 greys, the corners {0, 1, 127, 128, 254, 255}^3, colours built to have two or three equal
// fractions; in place; and the table facts: an identity table gives every byte back at N = 2, 4, 6, 16, 18 and stays
// within 1 at 17 and 33, the inverting table at N = 2 gives 255 - v, a table with two channels exchanged exchanges
// them, (0, 0, 0) maps to entry 0; grade_div255 against `/` for every argument below 65535.  Exit status 0: all held.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tr_grade.h"

static uint32_t g_x = 2463534242u;
static uint32_t rnd()
{
    g_x ^= g_x << 13, g_x ^= g_x >> 17, g_x ^= g_x << 5;
    return g_x;
}

// The rule for one pixel by the comparison chain: which of the six tetrahedra of the cell holds the point.
static void chain(int64_t n, const uint8_t *lut, const uint8_t *v, uint8_t *out)
{
    int64_t i[3], j[3], f[3];
    for (int x = 0; x < 3; x++) {
        const int64_t p = (int64_t)v[x] * (n - 1);
        i[x] = p / 255, f[x] = p % 255;
        j[x] = i[x] + 1 < n ? i[x] + 1 : n - 1;
    }
    auto entry = [&](int64_t r, int64_t g, int64_t b) { return lut + ((b * n + g) * n + r) * 3; };
    const int64_t fr = f[0], fg = f[1], fb = f[2];
    const uint8_t *V0 = entry(i[0], i[1], i[2]), *V3 = entry(j[0], j[1], j[2]), *V1, *V2;
    int64_t w0, w1, w2, w3;
    if (fr >= fg) {
        if (fg >= fb) {  // r >= g >= b
            V1 = entry(j[0], i[1], i[2]), V2 = entry(j[0], j[1], i[2]);
            w0 = 255 - fr, w1 = fr - fg, w2 = fg - fb, w3 = fb;
        } else if (fr >= fb) {  // r >= b > g
            V1 = entry(j[0], i[1], i[2]), V2 = entry(j[0], i[1], j[2]);
            w0 = 255 - fr, w1 = fr - fb, w2 = fb - fg, w3 = fg;
        } else {  // b > r >= g
            V1 = entry(i[0], i[1], j[2]), V2 = entry(j[0], i[1], j[2]);
            w0 = 255 - fb, w1 = fb - fr, w2 = fr - fg, w3 = fg;
        }
    } else {
        if (fb >= fg) {  // b >= g > r
            V1 = entry(i[0], i[1], j[2]), V2 = entry(i[0], j[1], j[2]);
            w0 = 255 - fb, w1 = fb - fg, w2 = fg - fr, w3 = fr;
        } else if (fb >= fr) {  // g > b >= r
            V1 = entry(i[0], j[1], i[2]), V2 = entry(i[0], j[1], j[2]);
            w0 = 255 - fg, w1 = fg - fb, w2 = fb - fr, w3 = fr;
        } else {  // g > r > b
            V1 = entry(i[0], j[1], i[2]), V2 = entry(j[0], j[1], i[2]);
            w0 = 255 - fg, w1 = fg - fr, w2 = fr - fb, w3 = fb;
        }
    }
    for (int c = 0; c < 3; c++) out[c] = (uint8_t)((w0 * V0[c] + w1 * V1[c] + w2 * V2[c] + w3 * V3[c] + 127) / 255);
}

static std::vector<uint8_t> identity(uint32_t n)
{
    std::vector<uint8_t> t(3 * (size_t)n * n * n);
    auto E = [&](uint32_t i) { return (uint8_t)((2u * 255u * i + (n - 1u)) / (2u * (n - 1u))); };
    for (uint32_t b = 0; b < n; b++)
        for (uint32_t g = 0; g < n; g++)
            for (uint32_t r = 0; r < n; r++) {
                uint8_t *e = &t[(((size_t)b * n + g) * n + r) * 3];
                e[0] = E(r), e[1] = E(g), e[2] = E(b);
            }
    return t;
}

int main()
{
    int bad = 0, cases = 0;
    for (uint32_t x = 0; x < 65535u; x++) bad += tr::grade_div255(x) != x / 255u;
    cases++;
    const uint32_t edges[] = { 2, 3, 17, 25, 26, 33 };
    const uint8_t corner[] = { 0, 1, 127, 128, 254, 255 };
    for (uint32_t n : edges) {
        std::vector<uint8_t> lut(3 * (size_t)n * n * n);
        for (uint8_t &e : lut) e = (uint8_t)(rnd() >> 24);
        std::vector<uint8_t> rgb;
        for (int k = 0; k < 20000 * 3; k++) rgb.push_back((uint8_t)(rnd() >> 24));
        for (int v = 0; v < 256; v++)
            for (int c = 0; c < 3; c++) rgb.push_back((uint8_t)v);
        for (uint8_t r : corner)
            for (uint8_t g : corner)
                for (uint8_t b : corner) rgb.push_back(r), rgb.push_back(g), rgb.push_back(b);
        // tied fractions: two or three channels share a value (equal fractions for every N), in every position
        for (int k = 0; k < 5000; k++) {
            const uint8_t a = (uint8_t)(rnd() >> 24), b = (uint8_t)(rnd() >> 24);
            const uint8_t t[4][3] = { { a, a, b }, { a, b, a }, { b, a, a }, { a, a, a } };
            for (int c = 0; c < 3; c++) rgb.push_back(t[k % 4][c]);
        }
        // ... and channels that differ by a whole number of cells: equal fractions, other indices (255 = (N - 1) k only)
        if (255u % (n - 1u) == 0u) {
            const uint32_t cell = 255u / (n - 1u);
            for (int k = 0; k < 2000; k++) {
                const uint32_t base = rnd() % cell, i0 = rnd() % (n - 1u), i1 = rnd() % (n - 1u), i2 = rnd() % (n - 1u);
                rgb.push_back((uint8_t)(i0 * cell + base)), rgb.push_back((uint8_t)(i1 * cell + base)), rgb.push_back((uint8_t)(i2 * cell + base));
            }
        }
        const size_t npx = rgb.size() / 3;
        std::vector<uint8_t> out(rgb.size(), 0xEE), want(rgb.size());
        tr::grade_host(npx, rgb.data(), out.data(), n, lut.data());
        for (size_t p = 0; p < npx; p++) chain(n, lut.data(), &rgb[3 * p], &want[3 * p]);
        bad += out != want;
        cases++;
        // in place
        std::vector<uint8_t> again = rgb;
        tr::grade_host(npx, again.data(), again.data(), n, lut.data());
        bad += again != want;
        cases++;
        // (0, 0, 0) is entry 0
        const uint8_t black[3] = { 0, 0, 0 };
        uint8_t c0[3];
        tr::grade_host(1, black, c0, n, lut.data());
        bad += memcmp(c0, lut.data(), 3) != 0;
        cases++;
    }
    // every colour of one channel against the others held, through identity tables
    std::vector<uint8_t> ramp;
    for (int v = 0; v < 256; v++) ramp.push_back((uint8_t)v), ramp.push_back((uint8_t)(255 - v)), ramp.push_back((uint8_t)((v * 7) & 255));
    for (int k = 0; k < 30000; k++) ramp.push_back((uint8_t)(rnd() >> 24));
    const uint32_t exact[] = { 2, 4, 6, 16, 18 }, near[] = { 17, 33 };
    for (uint32_t n : exact) {
        const std::vector<uint8_t> id = identity(n);
        std::vector<uint8_t> out(ramp.size());
        tr::grade_host(ramp.size() / 3, ramp.data(), out.data(), n, id.data());
        bad += out != ramp;
        cases++;
    }
    for (uint32_t n : near) {
        const std::vector<uint8_t> id = identity(n);
        std::vector<uint8_t> out(ramp.size());
        tr::grade_host(ramp.size() / 3, ramp.data(), out.data(), n, id.data());
        for (size_t k = 0; k < ramp.size(); k++) bad += out[k] > ramp[k] + 1 || out[k] + 1 < ramp[k];
        cases++;
    }
    {
        // N = 2: inversion, and red and blue exchanged
        std::vector<uint8_t> inv = identity(2), swp = identity(2), out(ramp.size());
        for (uint8_t &e : inv) e = (uint8_t)(255 - e);
        for (size_t k = 0; k < swp.size(); k += 3) {
            const uint8_t t = swp[k];
            swp[k] = swp[k + 2], swp[k + 2] = t;
        }
        tr::grade_host(ramp.size() / 3, ramp.data(), out.data(), 2, inv.data());
        for (size_t k = 0; k < ramp.size(); k++) bad += out[k] != 255 - ramp[k];
        tr::grade_host(ramp.size() / 3, ramp.data(), out.data(), 2, swp.data());
        for (size_t k = 0; k < ramp.size(); k += 3) bad += out[k] != ramp[k + 2] || out[k + 1] != ramp[k + 1] || out[k + 2] != ramp[k];
        cases += 2;
    }
    printf("%d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
