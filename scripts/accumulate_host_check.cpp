// accumulate_host_check.cpp -- the host half of frame accumulation (tr_accumulate.h: accumulate_divisor, accumulate_div,
// accumulate_host -- the body of tr_accumulate_host) as a stand-alone program, for a run under the host sanitizers.
// Needs no GPU and does not load the library:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Itiny_renderer_amd/csrc scripts/accumulate_host_check.cpp -o accumulate_host_check
//   ./accumulate_host_check
// (tests/test_accumulate.py builds it without the sanitizers and runs it for the division check.)
//   * the division: for every divisor D = 1 .. 8160 the multiplier and shift of accumulate_divisor give num / D at every
//     multiple of D and one below it up to the largest numerator 255 * D + D / 2, and at that numerator itself; for
//     D = 8160 and a few others at EVERY numerator;
//   * the rule: frames held in arrays of exactly n_bytes bytes (1, 7, 48 and 3 * 37 * 29 + 1: not multiples of 4), for
//     n = 1, 2, 3, 7, 8, 32 under equal (null), random, one-hot and all-255 weights, against num / D written with `/`;
//     a one-hot average is that frame byte for byte, an average of equal frames is the frame.
// Exit status 0: all held.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tr_accumulate.h"

int main()
{
    long bad = 0, points = 0;
    for (uint32_t D = 1; D <= tr::ACC_MAX_DIVISOR; D++) {
        const tr::AccDiv d = tr::accumulate_divisor(D);
        bad += d.half != D / 2u || d.mul == 0u || d.mul > (1u << 24);
        const uint32_t top = 255u * D + D / 2u;  // the largest numerator under this divisor
        for (uint32_t m = 0; m <= top; m += D) {
            bad += tr::accumulate_div(m, d) != m / D;
            if (m) bad += tr::accumulate_div(m - 1u, d) != (m - 1u) / D;
            points += 2;
        }
        bad += tr::accumulate_div(top, d) != top / D;
        bad += top / D != 255u;
    }
    for (uint32_t D : { 1u, 2u, 3u, 255u, 256u, 257u, 4095u, 4096u, 4097u, 7907u, 8159u, 8160u }) {
        const tr::AccDiv d = tr::accumulate_divisor(D);
        for (uint32_t m = 0; m <= tr::ACC_MAX_NUMERATOR; m++) bad += tr::accumulate_div(m, d) != m / D;
    }
    printf("division: %ld points, %ld mismatches so far\n", points, bad);

    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&x]() {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        return (uint32_t)(x >> 32);
    };
    const size_t sizes[] = { 1, 7, 48, 3 * 37 * 29 + 1 };
    const uint32_t counts[] = { 1, 2, 3, 7, 8, 32 };
    for (size_t n_bytes : sizes)
        for (uint32_t n : counts)
            for (int form = 0; form < 5; form++) {
                std::vector<std::vector<uint8_t>> frames(n, std::vector<uint8_t>(n_bytes));
                std::vector<const uint8_t *> ptrs(n);
                for (uint32_t k = 0; k < n; k++) {
                    for (uint8_t &b : frames[k]) b = form == 4 ? 255 : (uint8_t)rnd();
                    ptrs[k] = frames[k].data();
                }
                std::vector<uint32_t> w(n, 1u);
                const uint32_t hot = rnd() % n;
                if (form == 1)
                    for (uint32_t k = 0; k < n; k++) w[k] = k == hot ? 255u : rnd() % 4u == 0u ? 0u : rnd() % 256u;
                if (form == 2)
                    for (uint32_t k = 0; k < n; k++) w[k] = k == hot ? 1u + rnd() % 255u : 0u;
                if (form == 3 || form == 4) w.assign(n, 255u);
                std::vector<uint8_t> out(n_bytes, 0xAB);
                tr::accumulate_host(n_bytes, n, ptrs.data(), form == 0 ? nullptr : w.data(), out.data());
                uint32_t D = 0;
                for (uint32_t k = 0; k < n; k++) D += w[k];
                for (size_t b = 0; b < n_bytes; b++) {
                    uint32_t num = D / 2u;
                    for (uint32_t k = 0; k < n; k++) num += w[k] * frames[k][b];
                    bad += out[b] != num / D;
                }
                if (form == 2) bad += out != frames[hot];
                if (form == 4) bad += out != frames[0];
            }
    printf("%ld mismatches\n", bad);
    return bad ? 1 : 0;
}
