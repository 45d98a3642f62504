// tr_projector.h -- the rule of the projector (k_projector, tr_projector_host): an image of pw x ph pixels, rgb8 or rgba8,
// rows `stride` bytes apart with row 0 = top, is cast onto the DRAWN pixels of a finished colour frame from a second
// camera -- a slide projector, a decal, a light cookie, a second shadow-casting light.  Deferred: it reads the frame's
// colour and its z alone.  The matrix m (column-major) maps frame raster (x, y, z, 1) -- x right, y UP, z the frame's own
// depth at index x + y * W -- to projector raster (X, Y, Z, w).  For a drawn pixel (layer_drawn: bits(z) != bits(f32::MIN),
// the notion tr_ramp.h uses), in this order; a pixel that is not drawn, or that a step rejects, keeps its colour:
//   transform : X, Y, Z, w = ((m[i] x + m[4 + i] y) + m[8 + i] z) + m[12 + i], i = 0..3, x and y as f32 (exact), every
//               operation rounded once, nothing contracted: mul_m4_v4's order with the last factor 1.  Rejected unless
//               w > 0 and w is finite (a NaN fails the comparison).
//   divide    : r = 1.0f / w, correctly rounded, once; u = X r, v = Y r, zp = Z r.  Rejected unless 0 <= u <= pw - 1 and
//               0 <= v <= ph - 1 (a NaN fails).
//   position  : su = (int32)(u * 256.0f) -- the scaling is exact and the truncation a floor, u >= 0 --, ix = su >> 8,
//               ax = su & 255; likewise iy, ay.  Texel (ix, iy), y UP, is image row ph - 1 - iy.
//   image     : r, g, b and alpha (255 for rgb8) bilinearly by tr_warp.h's warp_weights and warp_round over the texels
//               (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1).  A texel of weight 0 is skipped and never loaded:
//               ix + 1 == pw goes with ax == 0 (u <= pw - 1), so no texel outside the image is ever read.
//   light     : f = 256 without PROJECTOR_OCCLUDE.  With it zo(i, j) is the occluder's depth at index i + j * pw, y UP, and
//               texel (i, j) is LIT iff !(zp + depth_bias < zo(i, j)): a NaN on either side is lit, an undrawn occluder
//               texel (f32::MIN) is lit.  Hard: f = 256 or 0 by the nearest texel (ix + (ax >= 128), iy + (ay >= 128)).
//               PROJECTOR_SOFT: f = (sum of the bilinear weights of the lit texels + 128) >> 8, weight-0 texels skipped.
//   blend     : coverage a = alpha * opacity (0..65280), a' = (a f + 128) >> 8; the pixel becomes tr_layer.h's
//               layer_px<mode>(sample, d, a').
// It follows: with m the identity, pw x ph = W x H and no OCCLUDE the result is the layer rule under LAYER_WHERE_DRAWN
// with the image at (0, 0); m[12], m[13] whole numbers move that layer; multiplying all of m by 2 changes nothing (every
// product and sum doubles exactly, r halves exactly, short of overflow); f = 256 leaves a.  Only colour changes.  A pixel
// depends on itself and the other inputs alone: the rule works in place.  One text for the device and the host compiler;
// only how an occluder texel is fetched differs (the device looks at the occluder's fast-clear flag first).
#pragma once

#include <stdint.h>
#include <string.h>

#include "tr_layer.h"
#include "tr_math.h"
#include "tr_ramp.h"
#include "tr_types.h"
#include "tr_warp.h"

namespace tr {

constexpr uint32_t PROJECTOR_OCCLUDE = 0x1u, PROJECTOR_SOFT = 0x2u;  // (= TR_PROJECTOR_OCCLUDE, TR_PROJECTOR_SOFT)
constexpr uint32_t PROJECTOR_MAX_SIDE = 8192u;

static_assert((PROJECTOR_MAX_SIDE - 1u) * 256u < (1u << 24), "a sample position is an exact f32 and fits i32");
static_assert(LAYER_FULL * 256u + 128u < (1u << 24), "coverage times light: operands and product within mul24");

// The numbers of a call: the header's tr_projector_params with the image's stride beside them; bpp = channels.
struct ProjectorRule {
    float m[16];
    uint32_t pw, ph, bpp, mode, opacity, flags, stride;
    float depth_bias;
};

// The bytes from the image's first to its last: what a call may read of `image`.
TR_HD int64_t projector_image_bytes(const ProjectorRule &q) { return (int64_t)q.stride * (int64_t)(q.ph - 1u) + (int64_t)q.pw * (int64_t)q.bpp; }

// Where a frame pixel falls in the projector's raster: the texel, the fractions in 1/256, the depth as the projector sees it.
struct ProjectorAt {
    int32_t ix, iy;
    uint32_t ax, ay;
    float zp;
};

// Steps transform, divide and position.  false: rejected.
TR_HD bool projector_at(const ProjectorRule &q, int32_t x, int32_t y, float z, ProjectorAt &h)
{
    const float fx = (float)x, fy = (float)y;
    float c[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        const float t0 = q.m[i] * fx, t1 = q.m[4 + i] * fy, t2 = q.m[8 + i] * z;
        const float s0 = t0 + t1;
        const float s1 = s0 + t2;
        c[i] = s1 + q.m[12 + i];
    }
    const float w = c[3];
    if (!(w > 0.0f && w <= 3.402823466e+38f)) return false;
    const float r = recip_of(w).y;
    const float u = c[0] * r, v = c[1] * r;
    h.zp = c[2] * r;
    if (!(u >= 0.0f && u <= (float)(q.pw - 1u) && v >= 0.0f && v <= (float)(q.ph - 1u))) return false;
    const int32_t su = (int32_t)(u * 256.0f), sv = (int32_t)(v * 256.0f);
    h.ix = su >> 8, h.ax = (uint32_t)su & 255u;
    h.iy = sv >> 8, h.ay = (uint32_t)sv & 255u;
    return true;
}

// Texel (i, j), y up, of the image: rgb in bits 0..23, alpha in 24..31 (255 for rgb8).  Bytes: any address, any stride.
TR_HD uint32_t projector_texel(const ProjectorRule &q, const uint8_t *image, int32_t i, int32_t j)
{
    const uint8_t *p = image + (size_t)(q.ph - 1u - (uint32_t)j) * (size_t)q.stride + (size_t)i * (size_t)q.bpp;
    const uint32_t a = q.bpp == 4u ? (uint32_t)p[3] : 255u;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | (a << 24);
}

// Step image: the bilinear sample, packed like a texel.
TR_HD uint32_t projector_sample(const ProjectorRule &q, const uint8_t *image, const ProjectorAt &h)
{
    const WarpWeights w = warp_weights(h.ax, h.ay);
    const uint32_t wt[4] = { w.w00, w.w10, w.w01, w.w11 };
    uint32_t sum[4] = { 0u, 0u, 0u, 0u };
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 4; t++) {
        if (wt[t] == 0u) continue;
        const uint32_t s = projector_texel(q, image, h.ix + (t & 1), h.iy + (t >> 1));
        sum[0] += wt[t] * (s & 0xFFu), sum[1] += wt[t] * ((s >> 8) & 0xFFu), sum[2] += wt[t] * ((s >> 16) & 0xFFu), sum[3] += wt[t] * (s >> 24);
    }
    return warp_round(sum[0]) | (warp_round(sum[1]) << 8) | (warp_round(sum[2]) << 16) | (warp_round(sum[3]) << 24);
}

// Is a texel whose occluder depth is zo lit for a pixel at zt = zp + depth_bias?
TR_HD bool projector_lit(float zt, float zo) { return !(zt < zo); }

// Step light: the fraction 0..256.  zo(i, j): the occluder's depth at texel (i, j), y up; called for texels inside the
// occluder only.
template <typename ZO>
TR_HD uint32_t projector_light(const ProjectorRule &q, const ProjectorAt &h, const ZO &zo)
{
    if (!(q.flags & PROJECTOR_OCCLUDE)) return 256u;
    const float zt = h.zp + q.depth_bias;
    if (!(q.flags & PROJECTOR_SOFT)) return projector_lit(zt, zo(h.ix + (h.ax >= 128u ? 1 : 0), h.iy + (h.ay >= 128u ? 1 : 0))) ? 256u : 0u;
    const WarpWeights w = warp_weights(h.ax, h.ay);
    const uint32_t wt[4] = { w.w00, w.w10, w.w01, w.w11 };
    uint32_t sum = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < 4; t++) {
        if (wt[t] == 0u) continue;
        if (projector_lit(zt, zo(h.ix + (t & 1), h.iy + (t >> 1)))) sum += wt[t];
    }
    return (sum + 128u) >> 8;
}

// Step blend's coverage: alpha * opacity under the light fraction f.
TR_HD uint32_t projector_coverage(uint32_t s, uint32_t opacity, uint32_t f) { return (mul24(mul24(s >> 24, opacity), f) + 128u) >> 8; }

// What frame pixel (x, y) with depth z blends: false if it keeps its colour, else the sample s and its coverage.
template <typename ZO>
TR_HD bool projector_source(const ProjectorRule &q, const uint8_t *image, const ZO &zo, int32_t x, int32_t y, float z, uint32_t &s, uint32_t &cov)
{
    if (!layer_drawn(z)) return false;
    ProjectorAt h;
    if (!projector_at(q, x, y, z, h)) return false;
    s = projector_sample(q, image, h);
    cov = projector_coverage(s, q.opacity, projector_light(q, h, zo));
    return true;
}

// The host's occluder: pw x ph floats, index i + j * pw.
struct ProjectorHostZ {
    const float *z;
    uint32_t pw;
    float operator()(int32_t i, int32_t j) const { return z[(size_t)j * pw + (size_t)i]; }
};

// The rule over a whole frame on the host (the body of tr_projector_host; the caller has checked the parameters).  rgb
// and out: W x H rgb8, row 0 = top; out may be rgb; z: index x + y * W, y up; occluder_z: only read under OCCLUDE.
inline void projector_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const ProjectorRule &q, const uint8_t *image,
                           const float *occluder_z, uint8_t *out)
{
    const size_t W = width, H = height;
    if (out != rgb) memmove(out, rgb, W * H * 3);
    const ProjectorHostZ zo = { occluder_z, q.pw };
    for (size_t r = 0; r < H; r++)
        for (size_t x = 0; x < W; x++) {
            const size_t y = H - 1 - r;
            uint32_t s = 0u, cov = 0u;
            if (!projector_source(q, image, zo, (int32_t)x, (int32_t)y, z[x + y * W], s, cov)) continue;
            uint8_t *o = out + (r * W + x) * 3;
            const uint32_t d = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
            const uint32_t v = layer_px_by(q.mode, s, d, cov);
            o[0] = (uint8_t)(v & 0xFFu), o[1] = (uint8_t)((v >> 8) & 0xFFu), o[2] = (uint8_t)((v >> 16) & 0xFFu);
        }
}

// k_projector's arguments, passed by value.  fb and out: rgb8, buffer row height - 1 - y; out is fb (in place) or does not
// overlap it, at any byte address.  fbclean / zclean: the frame's per-tile colour and z fast-clear flags over its 128 x 16
// tile grid (fbclean may be null: nothing is known).  z: the frame's depth, y up.  lower: null, or fbclean again -- in
// place a flagged tile that is stored whole has its flag lowered.  image: the image's bytes, any address; it overlaps
// neither buffer.  occ_z / occ_zclean: under OCCLUDE the occluder's depth (pw x ph, y up) and its z fast-clear flags over
// ITS tile grid, occ_ntx a row; a texel behind a raised flag counts as f32::MIN and its memory is not read.
struct ProjectorArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *lower;
    const float *z;
    const uint32_t *zclean;
    const uint8_t *image;
    const float *occ_z;
    const uint32_t *occ_zclean;
    uint32_t occ_ntx;
    DevFrame frame;
    ProjectorRule rule;
};

}  // namespace tr
