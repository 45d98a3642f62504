// warp_host_check.cpp -- the host half of the warp stage (tr_warp.h: warp_host -- the body of tr_warp_host -- and the inline
// functions k_warp calls) as a stand-alone program, for a run under the host sanitizers.  Needs no GPU and does not load
// the library:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Itiny_renderer_amd/csrc scripts/warp_host_check.cpp -o warp_host_check
//   ./warp_host_check
// It warps small random images held in arrays exactly as large as the function may touch (source, grid and output each
// a heap block of exactly its size), through random grids whose nodes reach several image sizes past every side and, in
// every grid, the two ends of the node range, under both edge modes, with one grid and with three, against a second
// formulation of the rule in 64-bit integers with floor division written out (`/` corrected for negatives) instead of
// shifts.  Then the rule's consequences: identity, flip, quarter turn, a constant frame under WARP_CLAMP.  Exit status 0:
// all held.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tr_warp.h"

static uint32_t g_x = 2463534242u;
static uint32_t rnd()
{
    g_x ^= g_x << 13, g_x ^= g_x >> 17, g_x ^= g_x << 5;
    return g_x;
}

static int64_t floor_div(int64_t a, int64_t b)  // b > 0
{
    int64_t q = a / b;
    if (a % b < 0) q--;
    return q;
}

static int64_t texel(int64_t W, int64_t H, const uint8_t *rgb, const tr::WarpRule &q, int64_t x, int64_t y, int c)
{
    if (q.edge == tr::WARP_CLAMP) {
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
    } else if (x < 0 || y < 0 || x >= W || y >= H) {
        return q.border[c];
    }
    return rgb[(y * W + x) * 3 + c];
}

// The rule from its words, every texel asked whatever its weight.
static void second(int64_t W, int64_t H, const uint8_t *rgb, int64_t Wd, int64_t Hd, const int32_t *grid, const tr::WarpRule &q, uint8_t *out)
{
    const int64_t gw = (Wd + 15) / 16 + 1, gh = (Hd + 15) / 16 + 1;
    for (int64_t Y = 0; Y < Hd; Y++)
        for (int64_t X = 0; X < Wd; X++)
            for (int c = 0; c < 3; c++) {
                const int32_t *g = grid + (q.per_channel ? c * gw * gh * 2 : 0);
                const int64_t gx = X / 16, fx = X % 16, gy = Y / 16, fy = Y % 16;
                int64_t s[2];
                for (int k = 0; k < 2; k++) {
                    const int64_t n00 = g[(gy * gw + gx) * 2 + k], n10 = g[(gy * gw + gx + 1) * 2 + k];
                    const int64_t n01 = g[((gy + 1) * gw + gx) * 2 + k], n11 = g[((gy + 1) * gw + gx + 1) * 2 + k];
                    s[k] = floor_div((16 - fx) * (16 - fy) * n00 + fx * (16 - fy) * n10 + (16 - fx) * fy * n01 + fx * fy * n11 + 128, 256);
                }
                const int64_t ix = floor_div(s[0], 256), ax = s[0] - 256 * ix, iy = floor_div(s[1], 256), ay = s[1] - 256 * iy;
                const int64_t acc = (256 - ax) * (256 - ay) * texel(W, H, rgb, q, ix, iy, c) + ax * (256 - ay) * texel(W, H, rgb, q, ix + 1, iy, c) +
                                    (256 - ax) * ay * texel(W, H, rgb, q, ix, iy + 1, c) + ax * ay * texel(W, H, rgb, q, ix + 1, iy + 1, c) + 32768;
                out[(Y * Wd + X) * 3 + c] = (uint8_t)(acc / 65536);
            }
}

static int g_failed = 0;
static void expect(bool ok, const char *what)
{
    if (!ok) {
        printf("FAILED: %s\n", what);
        g_failed++;
    }
}

int main()
{
    const uint32_t sizes[][4] = { { 1, 1, 1, 1 }, { 7, 5, 7, 5 }, { 7, 5, 17, 33 }, { 33, 18, 16, 16 }, { 2, 40, 49, 3 }, { 20, 20, 1, 35 } };
    long cases = 0;
    for (const auto &z : sizes) {
        const uint32_t W = z[0], H = z[1], Wd = z[2], Hd = z[3];
        const uint32_t gw = tr::warp_grid_side(Wd), gh = tr::warp_grid_side(Hd);
        for (uint32_t round = 0; round < 24; round++) {
            tr::WarpRule q;
            q.edge = round & 1u ? tr::WARP_CLAMP : tr::WARP_BORDER;
            q.per_channel = (round >> 1) & 1u;
            for (int c = 0; c < 3; c++) q.border[c] = round & 4u ? rnd() % 256u : 0u;
            const size_t n_nodes = (size_t)gw * gh * 2u * (q.per_channel ? 3u : 1u);
            // exact-size heap blocks: a read or write past any of them is the sanitizer's to find
            uint8_t *rgb = new uint8_t[(size_t)W * H * 3u];
            int32_t *grid = new int32_t[n_nodes];
            uint8_t *out = new uint8_t[(size_t)Wd * Hd * 3u], *want = new uint8_t[(size_t)Wd * Hd * 3u];
            for (size_t i = 0; i < (size_t)W * H * 3u; i++) rgb[i] = (uint8_t)rnd();
            const int32_t reach = (round < 12 ? 3 : 40) * 256 * (int32_t)(W > H ? W : H);
            for (size_t i = 0; i < n_nodes; i++) grid[i] = (int32_t)(rnd() % (uint32_t)(2 * reach + 1)) - reach + (int32_t)(256u * (W / 2u));
            grid[rnd() % n_nodes] = tr::WARP_NODE_MAX;
            grid[rnd() % n_nodes] = -tr::WARP_NODE_MAX;
            memset(out, 0xAA, (size_t)Wd * Hd * 3u);
            tr::warp_host(W, H, rgb, Wd, Hd, grid, q, out);
            second(W, H, rgb, Wd, Hd, grid, q, want);
            expect(memcmp(out, want, (size_t)Wd * Hd * 3u) == 0, "warp_host against the second formulation");
            cases++;
            delete[] rgb, delete[] grid, delete[] out, delete[] want;
        }
    }
    // consequences, 37 x 21
    {
        const uint32_t W = 37, H = 21, gw = tr::warp_grid_side(W), gh = tr::warp_grid_side(H);
        std::vector<uint8_t> rgb((size_t)W * H * 3u), out((size_t)W * H * 3u), turned((size_t)W * H * 3u);
        for (uint8_t &v : rgb) v = (uint8_t)rnd();
        std::vector<int32_t> ident((size_t)gw * gh * 2u), flip(ident.size());
        for (uint32_t gy = 0; gy < gh; gy++)
            for (uint32_t gx = 0; gx < gw; gx++) {
                ident[(gy * gw + gx) * 2u] = 256 * 16 * (int32_t)gx, ident[(gy * gw + gx) * 2u + 1u] = 256 * 16 * (int32_t)gy;
                flip[(gy * gw + gx) * 2u] = 256 * ((int32_t)W - 1 - 16 * (int32_t)gx), flip[(gy * gw + gx) * 2u + 1u] = 256 * 16 * (int32_t)gy;
            }
        tr::WarpRule q = { tr::WARP_BORDER, { 1u, 2u, 3u }, 0u };
        tr::warp_host(W, H, rgb.data(), W, H, ident.data(), q, out.data());
        expect(out == rgb, "the identity grid is a copy");
        tr::warp_host(W, H, rgb.data(), W, H, flip.data(), q, out.data());
        bool ok = true;
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++)
                for (uint32_t c = 0; c < 3; c++) ok = ok && out[(y * W + x) * 3u + c] == rgb[(y * W + (W - 1 - x)) * 3u + c];
        expect(ok, "a horizontal flip");
        // a quarter turn (np.rot90): the output is H wide and W high, out[Y][X] = F[X][W - 1 - Y]
        const uint32_t tw = tr::warp_grid_side(H), th = tr::warp_grid_side(W);
        std::vector<int32_t> turn((size_t)tw * th * 2u);
        for (uint32_t gy = 0; gy < th; gy++)
            for (uint32_t gx = 0; gx < tw; gx++)
                turn[(gy * tw + gx) * 2u] = 256 * ((int32_t)W - 1 - 16 * (int32_t)gy), turn[(gy * tw + gx) * 2u + 1u] = 256 * 16 * (int32_t)gx;
        tr::warp_host(W, H, rgb.data(), H, W, turn.data(), q, turned.data());
        ok = true;
        for (uint32_t Y = 0; Y < W; Y++)
            for (uint32_t X = 0; X < H; X++)
                for (uint32_t c = 0; c < 3; c++) ok = ok && turned[(Y * H + X) * 3u + c] == rgb[(X * W + (W - 1 - Y)) * 3u + c];
        expect(ok, "a quarter turn");
        // a constant frame under WARP_CLAMP, through a random grid
        for (size_t i = 0; i < rgb.size(); i++) rgb[i] = (uint8_t)(10u + 100u * (i % 3u));
        std::vector<int32_t> any(ident.size());
        for (int32_t &v : any) v = (int32_t)(rnd() % 60000u) - 30000;
        q.edge = tr::WARP_CLAMP;
        tr::warp_host(W, H, rgb.data(), W, H, any.data(), q, out.data());
        expect(out == rgb, "a constant frame stays constant under WARP_CLAMP");
    }
    printf("%ld random cases, %d failed\n", cases, g_failed);
    return g_failed ? 1 : 0;
}
