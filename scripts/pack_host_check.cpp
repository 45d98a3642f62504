// pack_host_check.cpp -- the host half of dynamic textures (tr_pack.h: pack_quad, the function k_pack_texels calls, run
// over an image by pack_image_host) as a stand-alone program, for a run under the host sanitizers.  Needs no GPU and
// does not load the library:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Itiny_renderer_amd/csrc scripts/pack_host_check.cpp -o pack_host_check
//   ./pack_host_check
// For images of 1 x 1, 7 x 5, 8 x 4 (whole quads: the 16-byte stores), 9 x 3 and 130 x 17 texels (partial quads, partial
// blocks of both block shapes, more than one 128 x 16 tile), a closure with a one-word set (phong) and the three with four-word sets, and which = 0..3, it
// replaces one image of a set built by pack_texels (tr_shaders.h, what tr_scene_create calls) and checks that the plain
// array and the set are, word for word, those of the four images with that one replaced -- also without a set, with
// some of the source's 128 x 16 tiles flagged clean (their texels are zeros, the source bytes there are poison) and with
// a logically cleared source (no source at all).  Every array is exactly as large as the rule may touch.  Exit status 0:
// all held.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tr_pack.h"

namespace {

uint32_t g_x = 2463534242u;
uint32_t rnd()
{
    g_x ^= g_x << 13;
    g_x ^= g_x >> 17;
    g_x ^= g_x << 5;
    return g_x;
}

}  // namespace

int main()
{
    int bad = 0, cases = 0;
    const uint32_t sizes[][2] = { { 1, 1 }, { 7, 5 }, { 8, 4 }, { 9, 3 }, { 130, 17 } };
    const int closures[] = { tr::FS_PHONG, tr::FS_SPECULAR, tr::FS_NORMAL_MAP, tr::FS_DARBOUX };
    for (const auto &wh : sizes)
        for (int fs : closures)
            for (uint32_t which = 0; which < 4; which++)
                for (int variant = 0; variant < 4; variant++) {  // 0: with a set, 1: without, 2: flagged tiles, 3: cleared source
                    const uint32_t w = wh[0], h = wh[1];
                    const size_t n = (size_t)w * h;
                    std::vector<uint32_t> img[4];
                    for (auto &v : img) {
                        v.resize(n);
                        for (uint32_t &t : v) t = rnd() & 0xFFFFFFu;
                    }
                    std::vector<uint8_t> src(3 * n);
                    for (uint8_t &b : src) b = (uint8_t)(rnd() >> 11);
                    const uint32_t ntx = (w + (uint32_t)tr::TILE_W - 1u) / (uint32_t)tr::TILE_W;
                    const uint32_t nty = (h + (uint32_t)tr::TILE_H - 1u) / (uint32_t)tr::TILE_H;
                    std::vector<uint32_t> clean((size_t)ntx * nty, 0u);
                    if (variant == 2)
                        for (size_t t = 0; t < clean.size(); t++) clean[t] = (t % 2u == 0u) ? 0xFFFFFFFFu : 0u;
                    // the image the call means: the source, zeros where a tile is flagged
                    std::vector<uint32_t> want(n);
                    for (uint32_t cy = 0; cy < h; cy++)
                        for (uint32_t cx = 0; cx < w; cx++) {
                            const size_t i = (size_t)cy * w + cx;
                            const bool zeros = variant == 3 || clean[((h - 1u - cy) / (uint32_t)tr::TILE_H) * ntx + cx / (uint32_t)tr::TILE_W] != 0u;
                            want[i] = zeros ? 0u : tr::pack_rgb8(src[3 * i], src[3 * i + 1], src[3 * i + 2]);
                        }
                    const uint32_t *before[4] = { img[0].data(), img[1].data(), img[2].data(), img[3].data() };
                    uint32_t bpr = 0;
                    std::vector<uint32_t> set = tr::pack_texels(fs, before, w, h, bpr);
                    const std::vector<uint32_t> set_before = set;
                    std::vector<uint32_t> plain = img[which];
                    tr::PackArgs a = {};
                    a.src = variant == 3 ? nullptr : src.data();
                    a.src_clean = variant == 2 ? clean.data() : nullptr;
                    a.src_all_clean = variant == 3 ? 1u : 0u;
                    a.texel = plain.data();
                    a.set = variant == 1 ? nullptr : set.data();
                    a.w = w;
                    a.h = h;
                    a.bpr = bpr;
                    a.fs = fs;
                    a.mode = a.set ? tr::pack_mode(fs, which) : 0u;
                    if (a.mode == tr::PACK_COLOUR && fs == tr::FS_SPECULAR) a.other = img[3].data();
                    if (a.mode == tr::PACK_SPEC) a.other = img[0].data();
                    tr::pack_image_host(a, tr::packed_words(fs));
                    img[which] = want;
                    const uint32_t *after[4] = { img[0].data(), img[1].data(), img[2].data(), img[3].data() };
                    uint32_t bpr2 = 0;
                    std::vector<uint32_t> set_want = tr::pack_texels(fs, after, w, h, bpr2);
                    if (variant == 1) set_want = set_before;  // (no set handed over: nothing of it is touched)
                    const int b0 = bad;
                    bad += plain != want;
                    bad += set != set_want || bpr != bpr2;
                    if (bad != b0) printf("mismatch: %u x %u, closure %d, which %u, variant %d\n", w, h, fs, which, variant);
                    cases++;
                }
    printf("%d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
