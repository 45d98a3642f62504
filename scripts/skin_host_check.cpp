// skin_host_check.cpp -- the host-only half of skinning (tr_skin.h: gather_skin_rows, skin_mesh_unrolled) as a
// stand-alone program, for a run under the host sanitizers.  Needs no GPU and does not load the library:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Itiny_renderer_amd/csrc -Itiny_renderer_amd/csrc/build scripts/skin_host_check.cpp -o skin_host_check
//   ./skin_host_check
// (tiny_renderer_amd/csrc/build/tr_powf_tables.inc is made by the library's Makefile.)
// It builds a small indexed mesh whose arrays are exactly as large as the functions may read, skins it under palettes
// of 1, 5 and 128 bones and checks the two contract cases: all-zero corners keep their bits under a palette of nan, a
// single influence of weight one equals xform_position / xform_normal.  Exit status 0: all held.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tr_skin.h"

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

int main()
{
    const uint32_t n_pos = 37, n_nrm = 29, n_tex = 11, n_tri = 301;  // (301 rows: no multiple of anything)
    std::vector<float> pos(3 * n_pos), nrm(3 * n_nrm);
    std::vector<uint32_t> idx(9 * (size_t)n_tri);
    for (uint32_t i = 0; i < 3 * n_pos; i++) pos[i] = i % 7 == 0 ? -0.0f : sinf(0.37f * (float)i);
    for (uint32_t i = 0; i < 3 * n_nrm; i++) nrm[i] = i % 5 == 0 ? -0.0f : cosf(0.53f * (float)i);
    for (uint32_t t = 0; t < n_tri; t++)
        for (uint32_t c = 0; c < 3; c++) {
            idx[9 * t + 3 * c] = (t * 5 + c * 11) % n_pos;
            idx[9 * t + 3 * c + 1] = (t + c) % n_tex;
            idx[9 * t + 3 * c + 2] = (t * 3 + c * 7) % n_nrm;
        }
    idx[0] = n_pos - 1;  // the last entries are read
    idx[2] = n_nrm - 1;
    int bad = 0;
    const uint32_t counts[] = { 1, 5, 128 };
    for (uint32_t n_bones : counts) {
        std::vector<uint32_t> bone(4 * (size_t)n_pos);
        std::vector<float> weight(4 * (size_t)n_pos);
        for (uint32_t p = 0; p < n_pos; p++)
            for (uint32_t j = 0; j < 4; j++) {
                bone[4 * p + j] = (p * 37 + j * 11) % n_bones;
                // position index 0 mod 3: no influence (zeros of either sign); 1 mod 3: one of weight one; else four
                weight[4 * p + j] = p % 3 == 0 ? (j & 1 ? -0.0f : 0.0f) : p % 3 == 1 ? (j == 2 ? 1.0f : 0.0f) : 0.1f + 0.2f * (float)j;
            }
        bone[4 * (n_pos - 1) + 3] = n_bones - 1;
        std::vector<float> pal(24 * (size_t)n_bones);
        for (size_t i = 0; i < pal.size(); i++) pal[i] = 0.3f * sinf(0.11f * (float)i) + (i % 24 == 0 || i % 24 == 5 || i % 24 == 10 ? 1.0f : 0.0f);
        std::vector<float> nan_pal(pal.size(), NAN);

        std::vector<uint32_t> rows((size_t)n_tri * tr::SKIN_ROW_WORDS);
        tr::gather_skin_rows(idx.data(), n_tri, bone.data(), weight.data(), rows.data());
        for (uint32_t t = 0; t < n_tri; t++)
            for (uint32_t c = 0; c < 3; c++)
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t P = idx[9 * t + 3 * c];
                    bad += rows[(size_t)t * 24 + 8 * c + 2 * j] != bone[4 * P + j];
                    bad += rows[(size_t)t * 24 + 8 * c + 2 * j + 1] != bits(weight[4 * P + j]);
                }

        std::vector<float> po(9 * (size_t)n_tri), no(9 * (size_t)n_tri), pn(9 * (size_t)n_tri), nn(9 * (size_t)n_tri);
        std::vector<uint32_t> io(9 * (size_t)n_tri);
        tr::skin_mesh_unrolled(pos.data(), nrm.data(), idx.data(), n_tri, bone.data(), weight.data(), pal.data(), po.data(), no.data(), io.data());
        tr::skin_mesh_unrolled(pos.data(), nrm.data(), idx.data(), n_tri, bone.data(), weight.data(), nan_pal.data(), pn.data(), nn.data(), io.data());
        for (uint32_t t = 0; t < n_tri; t++)
            for (uint32_t c = 0; c < 3; c++) {
                const uint32_t k = 3 * t + c, P = idx[9 * t + 3 * c], N = idx[9 * t + 3 * c + 2];
                bad += io[3 * k] != k || io[3 * k + 1] != idx[9 * t + 3 * c + 1] || io[3 * k + 2] != k;
                if (P % 3 == 0)
                    for (int r = 0; r < 3; r++) bad += bits(pn[3 * k + r]) != bits(pos[3 * P + r]) || bits(nn[3 * k + r]) != bits(nrm[3 * N + r]);
                if (P % 3 == 1) {
                    const float *e = &pal[24 * (size_t)bone[4 * P + 2]];
                    float x = pos[3 * P], y = pos[3 * P + 1], z = pos[3 * P + 2], a = nrm[3 * N], b = nrm[3 * N + 1], d = nrm[3 * N + 2];
                    tr::xform_position(e, x, y, z);
                    tr::xform_normal(e + 12, a, b, d);
                    bad += bits(po[3 * k]) != bits(x) || bits(po[3 * k + 1]) != bits(y) || bits(po[3 * k + 2]) != bits(z);
                    bad += bits(no[3 * k]) != bits(a) || bits(no[3 * k + 1]) != bits(b) || bits(no[3 * k + 2]) != bits(d);
                }
                if (P % 3 == 2)
                    for (int r = 0; r < 3; r++) bad += !isnan(pn[3 * k + r]) || !isnan(nn[3 * k + r]) || isnan(po[3 * k + r]);
            }
        printf("%u bones: %d mismatches so far\n", n_bones, bad);
    }
    return bad ? 1 : 0;
}
