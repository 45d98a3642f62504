// tr_morph.h -- the arithmetic of morph targets (k_morph, tr_morph_mesh): a pose is a weight per target, and every
// position and normal component p with deltas d_0 .. d_{T-1} becomes
//     v = p;  for k = 0 .. T-1, skipping every k with w[k] == 0.0f (either sign):  v = fl(v + fl(w[k] * d_k))
// -- one multiply and one add per step, each rounded once (the library is built with -ffp-contract=off).  The skip is
// part of the rule: under a pose of zeros every component is the mesh's own bit pattern (-0.0 stays -0.0, and a target
// that holds inf or nan does nothing at weight zero).  One function for the device and the host compiler, so that both
// see the same text.
#pragma once

#include <stdint.h>

#include "tr_math.h"

namespace tr {

// One step of the rule for one component: the caller has found w != 0.
TR_HD float morph_step(float v, float w, float d)
{
    const float t = w * d;
    return v + t;
}

// The whole rule for one component on the host: deltas d[k * stride], k = 0 .. n_targets - 1.
inline float morph_component(float p, uint32_t n_targets, const float *w, const float *d, size_t stride)
{
    float v = p;
    for (uint32_t k = 0; k < n_targets; k++)
        if (w[k] != 0.0f) v = morph_step(v, w[k], d[(size_t)k * stride]);
    return v;
}

// k_morph's per-frame table, passed by value: frame f of a launch blends under weights w[f] (n_targets floats in device
// memory) into dst[f] (n_rows x TRI_FLOATS floats).
constexpr int MORPH_MAX_FRAMES = 32;  // (= plan::GROUP_MAX)
struct MorphFrame {
    const float *w;
    float *dst;
};
struct MorphTable {
    MorphFrame f[MORPH_MAX_FRAMES];
};

}  // namespace tr
