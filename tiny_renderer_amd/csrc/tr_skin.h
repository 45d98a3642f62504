// tr_skin.h -- the arithmetic of skinning (k_skin, tr_skin_mesh).  A skin gives every POSITION INDEX of the mesh
// SKIN_INFLUENCES = 4 pairs (bone index, weight); a palette is one tr_instance_xform (24 floats: m[12] for positions,
// n[9] for normals, 3 unused) per bone.  Corner i of a polygon, position p at position index P, normal a at its own
// normal index (OBJ indexes normals separately, so a normal has no influences of its own: it takes those of P):
//     acc = none
//     for j = 0 .. 3, in this order, skipping every j with weight[P][j] == 0.0f (either sign):
//         q   = xform_position(palette[bone[P][j]].m, p)             -- tr_shaders.h, unchanged
//         t_r = fl(weight[P][j] * q_r)                               -- r = 0 .. 2
//         acc_r = (acc is none) ? t_r : fl(acc_r + t_r)
//     p' = (acc is none) ? p : acc
// and the normal likewise with xform_normal(palette[..].n, a).  Every product and every sum is rounded once (the library
// is built with -ffp-contract=off); weights are used as given, normals are not renormalised.  The skip is part of the
// rule: a corner whose four weights are zero keeps the mesh's own bit patterns (-0.0 stays -0.0, and a palette that
// holds inf or nan does nothing to it), and a corner with one influence of weight 1.0f gets exactly the bits of
// xform_position / xform_normal -- what a transform table of that one entry draws.  One text for the device and the
// host compiler; only where the 24 floats of a bone come from differs (k_skin: LDS, the host: the caller's array).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "tr_shaders.h"

namespace tr {

constexpr int SKIN_INFLUENCES = 4;  // (= TR_SKIN_INFLUENCES)
constexpr int SKIN_MAX_BONES = 128; // (= TR_SKIN_MAX_BONES)
// The influences as k_skin reads them: one row per polygon, 3 corners x 4 x {bone index, weight} = 24 words (six
// 16-byte pieces); word 8 c + 2 j is corner c's j-th bone index, word 8 c + 2 j + 1 the bits of its weight.
constexpr int SKIN_ROW_WORDS = 3 * SKIN_INFLUENCES * 2;

// The rule for one corner.  `entry(b, e)` fills e[0 .. 24) with the palette's entry of bone b; bone / weight: the four
// influences of the corner's position index; p, a: the corner's position and normal, replaced.  All indices are
// compile-time constants once the loops are unrolled.
template <typename Entry>
TR_HD void skin_corner(const Entry &entry, const uint32_t *bone, const float *weight, float *p, float *a)
{
    float ap[3] = { 0.0f, 0.0f, 0.0f }, an[3] = { 0.0f, 0.0f, 0.0f };
    bool have = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < SKIN_INFLUENCES; j++) {
        const float w = weight[j];
        if (w != 0.0f) {
            float e[INST_XFORM_FLOATS];
            entry(bone[j], e);
            float x = p[0], y = p[1], z = p[2];
            xform_position(e, x, y, z);
            float u = a[0], v = a[1], s = a[2];
            xform_normal(e + 12, u, v, s);
            const float tp[3] = { w * x, w * y, w * z };
            const float tn[3] = { w * u, w * v, w * s };
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int r = 0; r < 3; r++) {
                ap[r] = have ? ap[r] + tp[r] : tp[r];
                an[r] = have ? an[r] + tn[r] : tn[r];
            }
            have = true;
        }
    }
    if (have) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int r = 0; r < 3; r++) {
            p[r] = ap[r];
            a[r] = an[r];
        }
    }
}

// A palette in the caller's memory: n_bones x 24 floats.
struct HostPalette {
    const float *pal;
    TR_HD void operator()(uint32_t b, float *e) const
    {
        for (int i = 0; i < INST_XFORM_FLOATS; i++) e[i] = pal[(size_t)INST_XFORM_FLOATS * b + i];
    }
};

// The influence rows of a mesh (host): row t of `out` (SKIN_ROW_WORDS words) holds, per corner of polygon t, the four
// influences of the corner's position index -- idx: 9 indices per polygon (position, texture, normal per corner);
// bone / weight: 4 per position index.
inline void gather_skin_rows(const uint32_t *idx, uint32_t n_tri, const uint32_t *bone, const float *weight, uint32_t *out)
{
    for (uint32_t t = 0; t < n_tri; t++)
        for (int c = 0; c < 3; c++) {
            const size_t P = idx[9u * (size_t)t + 3u * (size_t)c];
            for (int j = 0; j < SKIN_INFLUENCES; j++) {
                uint32_t wbits;
                memcpy(&wbits, &weight[P * SKIN_INFLUENCES + j], sizeof wbits);
                out[(size_t)t * SKIN_ROW_WORDS + 8 * c + 2 * j] = bone[P * SKIN_INFLUENCES + j];
                out[(size_t)t * SKIN_ROW_WORDS + 8 * c + 2 * j + 1] = wbits;
            }
        }
}

// The skinned mesh on the host, unrolled: corner 3 t + i of polygon t gets a position and a normal of its own (a normal
// that corners with different positions share gets different results), idx_out = {3 t + i, the corner's texture index,
// 3 t + i}.  pos_out, nrm_out, idx_out: n_tri * 9 each.  The caller has checked every bone index against the palette.
inline void skin_mesh_unrolled(const float *pos, const float *nrm, const uint32_t *idx, uint32_t n_tri, const uint32_t *bone,
                               const float *weight, const float *palette, float *pos_out, float *nrm_out, uint32_t *idx_out)
{
    const HostPalette entry = { palette };
    for (uint32_t t = 0; t < n_tri; t++)
        for (uint32_t i = 0; i < 3u; i++) {
            const uint32_t *ix = idx + 9u * (size_t)t + 3u * i;
            const size_t c = 3u * (size_t)t + i, P = ix[0], N = ix[2];
            float p[3] = { pos[3u * P], pos[3u * P + 1u], pos[3u * P + 2u] };
            float a[3] = { nrm[3u * N], nrm[3u * N + 1u], nrm[3u * N + 2u] };
            skin_corner(entry, bone + P * SKIN_INFLUENCES, weight + P * SKIN_INFLUENCES, p, a);
            for (int r = 0; r < 3; r++) {
                pos_out[3u * c + r] = p[r];
                nrm_out[3u * c + r] = a[r];
            }
            idx_out[3u * c] = (uint32_t)c;
            idx_out[3u * c + 1u] = ix[1];
            idx_out[3u * c + 2u] = (uint32_t)c;
        }
}

// k_skin's per-frame table, passed by value: frame f of a launch skins the rows src[f] under the palette pal[f]
// (n_bones x 24 floats in device memory, 16-byte aligned) into dst[f]; src may be dst.
constexpr int SKIN_MAX_FRAMES = 32;  // (= plan::GROUP_MAX)
struct SkinFrame {
    const float *pal;
    const float *src;
    float *dst;
};
struct SkinTable {
    SkinFrame f[SKIN_MAX_FRAMES];
};

}  // namespace tr
