// tr_pack.h -- the rule of dynamic textures (k_pack_texels, tr_scene_set_texture*): image `which` of a scene is replaced
// by a w x h image of tightly packed rgb8 rows (row 0 = top), and BOTH of the scene's representations follow:
//   * the plain array d_texel[which]: one word per texel, r | g << 8 | b << 16 (alpha 0), row by row;
//   * the texel set of the scene's closure `fs` (tr_texels.h), where the scene has one -- exactly the words that depend
//     on image `which`:
//         word 0's low 24 bits   for which == 0,
//         word 0's top byte      for which == 3 under FS_SPECULAR,
//         words 1..3             for which == packed_normal_source(fs): decode_normal of the new texel,
//     and nothing else.  Word 0 is rebuilt whole from the new texel and the OTHER image's plain array (the specular map's
//     byte, or the colour image's colour): pack_word0 is pack_texels' own expression.  Padding texels of partial blocks
//     stay zero.
// A lane of the kernel owns four horizontally adjacent texels -- a QUAD, pack_quad below: 16 contiguous bytes of the
// plain array, 16 contiguous bytes of an 8 x 4 block (one-word sets), 64 contiguous bytes of a 4 x 2 block (four-word
// sets); packed_index places them.  The host runs the same function over the quads of an image (pack_image_host), so
// that both compilers see one text.  decode_normal is the plain IEEE form (tr_shaders.h) on both sides.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "tr_shaders.h"
#include "tr_texels.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t PACK_QUAD = 4;  // texels a lane owns

// What a call on image `which` touches in the set of closure `fs`
constexpr uint32_t PACK_COLOUR = 1u;  // word 0, from the new colour texel and the specular map's plain array
constexpr uint32_t PACK_SPEC = 2u;    // word 0, from the colour image's plain array and the new specular texel
constexpr uint32_t PACK_NORMAL = 4u;  // words 1..3
TR_HD uint32_t pack_mode(int fs, uint32_t which)
{
    if (which == 0u) return PACK_COLOUR;
    if (which == 3u && fs == FS_SPECULAR) return PACK_SPEC;
    if ((int)which == packed_normal_source(fs)) return PACK_NORMAL;
    return 0u;
}

// the plain array's word of an rgb8 texel
TR_HD uint32_t pack_rgb8(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16); }

// word 0 of a set's texel (pack_texels, tr_shaders.h)
TR_HD uint32_t pack_word0(int fs, uint32_t colour, uint32_t spec) { return (colour & 0xFFFFFFu) | (fs == FS_SPECULAR ? (spec & 0xFFu) << 24 : 0u); }

// What k_pack_texels gets.  `src`: the new image; src_clean (may be null): the colour-clean flags of the frame `src`
// is, one word per 128 x 16 tile of a whole frame of w x h pixels, rows counted from the BOTTOM as the frame's tiles
// are -- a tile whose flag is up is not read and counts as zeros; src_all_clean: every tile does (a logically cleared
// frame).  `other`: the plain array word 0 is completed from (PACK_COLOUR under FS_SPECULAR: image 3's; PACK_SPEC:
// image 0's), else null.
struct PackArgs {
    const uint8_t *src;
    const uint32_t *src_clean;
    uint32_t *texel;        // d_texel[which]
    uint32_t *set;          // the texel set, or null
    const uint32_t *other;
    uint32_t w, h;
    uint32_t bpr;           // blocks per row of the set
    uint32_t mode;          // pack_mode(fs, which); 0 with a set: the plain array alone
    int32_t fs;
    uint32_t src_all_clean;
};

// One quad: texels (cx .. cx + n - 1, cy), cx a multiple of 4, 1 <= n <= 4, from their plain words t[0..4) (zeros beyond
// n) and the other image's o[0..4) (where the mode needs them, else null).  WORDS: words per texel of the set (1 or 4).
// WIDE: the image's width is a multiple of 4 (so n == 4) and the plain array 16-byte aligned -- its four words are one
// store.  Writes n words of the plain array and the set's words the mode owns; in a one-word set the quad is one 16-byte
// store whose words beyond n are the zeros the padding holds anyway, in a four-word set nothing beyond texel n - 1 is
// written.
template <int WORDS, bool WIDE>
TR_HD void pack_quad(const PackArgs &a, uint32_t cx, uint32_t cy, uint32_t n, const uint32_t *t, const uint32_t *o)
{
    uint32_t *plain = a.texel + ((size_t)cy * a.w + cx);
    if (WIDE) {
        *reinterpret_cast<Texel4 *>(plain) = Texel4{ t[0], t[1], t[2], t[3] };
    } else {
        for (uint32_t k = 0; k < PACK_QUAD; k++)
            if (k < n) plain[k] = t[k];
    }
    if (!a.set || a.mode == 0u) return;
    // (cx is a multiple of 4 and both block widths are: the quad's texels are consecutive in the tiled order, and the
    // set -- whole 128-byte blocks -- is 16-byte aligned there)
    uint32_t *q = a.set + (size_t)packed_index(WORDS, a.bpr, cx, cy) * WORDS;
    if (WORDS == 1) {
        if (a.mode == PACK_COLOUR)  // (a one-word set has no other word and no closure with a specular byte)
            *reinterpret_cast<Texel4 *>(q) = Texel4{ pack_word0(a.fs, t[0], 0u), pack_word0(a.fs, t[1], 0u), pack_word0(a.fs, t[2], 0u),
                                                     pack_word0(a.fs, t[3], 0u) };
        return;
    }
    for (uint32_t k = 0; k < PACK_QUAD; k++) {
        if (k >= n) break;
        if (a.mode == PACK_COLOUR) q[k * WORDS] = pack_word0(a.fs, t[k], o ? o[k] : 0u);
        if (a.mode == PACK_SPEC) q[k * WORDS] = pack_word0(a.fs, o[k], t[k]);
        if (a.mode == PACK_NORMAL) {
            const vec3 nrm = decode_normal(t[k]);
            q[k * WORDS + 1] = f32_bits(nrm.x);
            q[k * WORDS + 2] = f32_bits(nrm.y);
            q[k * WORDS + 3] = f32_bits(nrm.z);
        }
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The rule over a whole image on the host: what one launch of k_pack_texels leaves in a.texel and a.set (a.src_clean
// and a.src_all_clean are honoured).  words: packed_words(fs) (any value with a.set null).
inline void pack_image_host(const PackArgs &a, int words)
{
    const uint32_t tiles_x = (a.w + (uint32_t)TILE_W - 1u) / (uint32_t)TILE_W;
    const bool wide = a.w % PACK_QUAD == 0u && (uintptr_t)a.texel % 16u == 0u;  // (the launcher's choice)
    for (uint32_t cy = 0; cy < a.h; cy++)
        for (uint32_t cx = 0; cx < a.w; cx += PACK_QUAD) {
            const uint32_t n = a.w - cx < PACK_QUAD ? a.w - cx : PACK_QUAD;
            const uint32_t y = a.h - 1u - cy;  // the frame's row, counted from the bottom
            const bool zeros = a.src_all_clean || (a.src_clean && a.src_clean[(y / (uint32_t)TILE_H) * tiles_x + cx / (uint32_t)TILE_W] != 0u);
            uint32_t t[PACK_QUAD] = {}, o[PACK_QUAD] = {};
            for (uint32_t k = 0; k < n; k++) {
                const size_t i = (size_t)cy * a.w + cx + k;
                if (!zeros) t[k] = pack_rgb8(a.src[3 * i], a.src[3 * i + 1], a.src[3 * i + 2]);
                if (a.other) o[k] = a.other[i];
            }
            const uint32_t *op = a.other ? o : nullptr;
            if (words == 4) wide ? pack_quad<4, true>(a, cx, cy, n, t, op) : pack_quad<4, false>(a, cx, cy, n, t, op);
            else wide ? pack_quad<1, true>(a, cx, cy, n, t, op) : pack_quad<1, false>(a, cx, cy, n, t, op);
        }
}
#endif

}  // namespace tr
