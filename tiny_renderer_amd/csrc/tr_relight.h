// tr_relight.h -- the rule of relighting (k_relight, tr_relight_host, tr_relight_normals_host): coloured directional,
// point and spot lights with a highlight laid on a finished colour frame from its own depth.  Deferred: it reads the
// frame's colour (rgb8, row 0 = top), its z (index x + y * W, y UP) and the numbers of the call alone.  u (column-major)
// maps frame raster (x, y, z, 1) to model space: the view's i_vpmv (tr_prepare_uniforms kind 2).  Every f32 operation is
// rounded once, in the order written; nothing is contracted; '/' and sqrt are IEEE's.
//   position(x, y) : for a pixel inside the frame that is drawn (layer_drawn(z)).  c[i] = ((u[i] x + u[4 + i] y) +
//              u[8 + i] z) + u[12 + i], i = 0..3, x and y as f32 (exact): projector_at's order.  Accepted iff w = c[3] is
//              finite and not 0; then r = recip_of(w).y and P = (c0 r, c1 r, c2 r), accepted only if all three are finite.
//              A pixel outside the frame, not drawn or not accepted has no position.  (A depth that is NaN or infinite
//              never has one: it makes every c[i] NaN or the product non-finite.)
//   normal(x, y) : for a pixel with a position P and depth zc.  Horizontally the candidates are a = (x + 1, y) and
//              b = (x - 1, y); a candidate is usable iff it has a position.  Both usable: a iff |za - zc| <= |zb - zc| (a NaN
//              makes the comparison false and takes b); one usable: that one; none: no normal.  dx = P(a) - P or
//              dx = P - P(b): the difference always points towards +x.  The same vertically with (x, y + 1) and (x, y - 1)
//              gives dy.  N = cross3(dx, dy), V = sub3(eye, P); if dot3(N, V) < 0 then N = -N.  No normal unless dot3(N, N)
//              is finite and > 0 and dot3(N, V) is not NaN, and none if dot3(V, V) is 0 or not finite.  n = normalize3(N),
//              v = normalize3(V).
//   light l  : RELIGHT_DIRECTIONAL: L = dir (the host gives a unit vector towards the light), att = 1.  RELIGHT_POINT:
//              D = sub3(pos, P), d2 = dot3(D, D); skipped unless d2 is finite and > 0; L = normalize3(D),
//              att = recip_of(1.0f + falloff * d2).y.  RELIGHT_SPOT: a point light with c = dot3(-L, dir) (dir: the unit
//              axis, from the lamp along its beam), cone = min(1, max(0, (c - cos_outer) * cone_scale)) with a NaN giving
//              0, att = att * cone.  diff = dot3(n, L); the light adds nothing unless diff > 0 (a NaN fails).  Only if
//              specular > 0: h = normalize3(add3(L, v)), s = max(0, dot3(n, h)) (a NaN gives 0), s = s * s done
//              shininess_log2 times (0..10: the exponent 2^k exactly, no powf), diff = diff + specular * s.
//              e = (diff * att) * intensity; q = f32_to_u32((e > 16 ? 16 : e) * 256.0f): 0..4096 in units of 1/256, a NaN
//              gives 0.  Per channel acc[c] += q * colour[c], in u32.
//   sample   : per channel s[c] = min(255, (256 * ambient[c] + acc[c] + 128) >> 8).  With RELIGHT_SHOW_NORMALS instead
//              s[c] = f32_to_u8((n[c] * 0.5f + 0.5f) * 255.0f) and the lights are ignored: a normal map of the picture.
//              Then with RELIGHT_ALBEDO s = layer_px<MULTIPLY>(s, d, LAYER_FULL), d the pixel's own colour: under ADD the
//              result is d + d * s, a coloured light on an already shaded picture; plain MULTIPLY lights an unshaded one.
//   blend    : the pixel becomes tr_layer.h's layer_px_by(mode, s, d, 255 * opacity), opacity 0..256.
// A pixel that is not drawn, has no position or has no normal KEEPS its colour.  Only colour changes: z, winner words and
// the shadow buffer are never written.  A pixel reads its own colour but its neighbours' DEPTH only: the rule works in
// place without a scratch frame, in any order of the pixels.  One text for the device and the host compiler; only where
// a neighbour's position comes from differs (k_relight: LDS, computed once per staged pixel; the host: an array).
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "tr_layer.h"
#include "tr_math.h"
#include "tr_types.h"

namespace tr {

constexpr uint32_t RELIGHT_MAX_LIGHTS = 8u;                                          // (= TR_RELIGHT_MAX_LIGHTS)
constexpr uint32_t RELIGHT_DIRECTIONAL = 0u, RELIGHT_POINT = 1u, RELIGHT_SPOT = 2u;  // (= TR_LIGHT_DIRECTIONAL ..)
constexpr uint32_t RELIGHT_ALBEDO = 0x1u, RELIGHT_SHOW_NORMALS = 0x2u;               // (= TR_RELIGHT_ALBEDO ..)
constexpr uint32_t RELIGHT_MAX_SHININESS_LOG2 = 10u;
constexpr uint32_t RELIGHT_MAX_LEVEL = 4096u;  // 16 in units of 1/256

static_assert(RELIGHT_MAX_LEVEL < (1u << 24) && RELIGHT_MAX_LIGHTS * RELIGHT_MAX_LEVEL * 255u < (1u << 24),
              "a level times a channel is a mul24, and eight of them stay far inside a u32");
static_assert((uint64_t)RELIGHT_MAX_LIGHTS * RELIGHT_MAX_LEVEL * 255u + 256u * 255u + 128u < (1ull << 32), "the sample's sum fits a u32");

// A light: the header's tr_light, field by field (64 bytes).
struct RelightLight {
    uint32_t kind;
    float pos[3];  // POINT, SPOT
    float dir[3];  // DIRECTIONAL: towards the light; SPOT: the axis, from the lamp along the beam
    uint8_t colour[4];
    float intensity, falloff, cos_outer, cone_scale, specular;
    uint32_t shininess_log2;
    uint32_t reserved[2];
};
static_assert(sizeof(RelightLight) == 64, "tr_light");

// The numbers of a call: the header's tr_relight_params with the ambient colour packed (r in bits 0..7, g 8..15, b
// 16..23) and the lights beside them.
struct RelightRule {
    float u[16];
    float eye[3];
    uint32_t ambient, mode, opacity, flags, n_lights;
    RelightLight lights[RELIGHT_MAX_LIGHTS];
};

TR_HD bool relight_finite(float v) { return (f32_bits(v) & 0x7F800000u) != 0x7F800000u; }

// Step position for a pixel inside the frame.  false: none.
TR_HD bool relight_position(const float *u, int32_t x, int32_t y, float z, vec3 &P)
{
    if (!layer_drawn(z)) return false;
    const float fx = (float)x, fy = (float)y;
    float c[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        const float t0 = u[i] * fx, t1 = u[4 + i] * fy, t2 = u[8 + i] * z;
        const float s0 = t0 + t1;
        const float s1 = s0 + t2;
        c[i] = s1 + u[12 + i];
    }
    const float w = c[3];
    if (!relight_finite(w) || w == 0.0f) return false;
    const float r = recip_of(w).y;
    P = make3(c[0] * r, c[1] * r, c[2] * r);
    return relight_finite(P.x) && relight_finite(P.y) && relight_finite(P.z);
}

// A pixel as its neighbours see it: has it a position, which, and its depth.
struct RelightTap {
    bool ok;
    vec3 P;
    float z;
};

// One axis of step normal: the difference towards + from the centre c and the candidates a (+) and b (-).  false: none.
TR_HD bool relight_difference(const RelightTap &c, const RelightTap &a, const RelightTap &b, vec3 &d)
{
    bool use_a;
    if (a.ok && b.ok) use_a = fabsf(a.z - c.z) <= fabsf(b.z - c.z);
    else if (a.ok) use_a = true;
    else if (b.ok) use_a = false;
    else return false;
    d = use_a ? sub3(a.P, c.P) : sub3(c.P, b.P);
    return true;
}

// Step normal: n and v of the centre c from its four neighbours (xa = (x + 1, y), xb = (x - 1, y), ya = (x, y + 1),
// yb = (x, y - 1)).  false: none.
TR_HD bool relight_normal(const float *eye, const RelightTap &c, const RelightTap &xa, const RelightTap &xb, const RelightTap &ya,
                          const RelightTap &yb, vec3 &n, vec3 &v)
{
    if (!c.ok) return false;
    vec3 dx, dy;
    if (!relight_difference(c, xa, xb, dx) || !relight_difference(c, ya, yb, dy)) return false;
    vec3 N = cross3(dx, dy);
    const vec3 V = sub3(make3(eye[0], eye[1], eye[2]), c.P);
    const float nv = dot3(N, V);
    if (nv < 0.0f) N = make3(-N.x, -N.y, -N.z);
    const float nn = dot3(N, N), vv = dot3(V, V);
    if (!(nn > 0.0f) || !relight_finite(nn) || nv != nv) return false;
    if (!(vv > 0.0f) || !relight_finite(vv)) return false;
    n = normalize3(N);
    v = normalize3(V);
    return true;
}

// Step light: what light l adds to acc at a point P with unit normal n and unit direction v to the eye.
TR_HD void relight_light(const RelightLight &l, vec3 P, vec3 n, vec3 v, uint32_t acc[3])
{
    vec3 L = make3(l.dir[0], l.dir[1], l.dir[2]);
    float att = 1.0f;
    if (l.kind != RELIGHT_DIRECTIONAL) {
        const vec3 D = sub3(make3(l.pos[0], l.pos[1], l.pos[2]), P);
        const float d2 = dot3(D, D);
        if (!(d2 > 0.0f) || !relight_finite(d2)) return;
        const vec3 axis = L;
        L = normalize3(D);
        const float t = l.falloff * d2;
        att = recip_of(1.0f + t).y;
        if (l.kind == RELIGHT_SPOT) {
            const float c = dot3(make3(-L.x, -L.y, -L.z), axis);
            const float ramp = (c - l.cos_outer) * l.cone_scale;
            const float cone = ramp > 0.0f ? (ramp < 1.0f ? ramp : 1.0f) : 0.0f;  // (a NaN: 0)
            att = att * cone;
        }
    }
    float diff = dot3(n, L);
    if (!(diff > 0.0f)) return;
    if (l.specular > 0.0f) {
        const vec3 h = normalize3(add3(L, v));
        const float nh = dot3(n, h);
        float s = nh > 0.0f ? nh : 0.0f;  // (a NaN: 0)
        for (uint32_t k = 0; k < l.shininess_log2; k++) s = s * s;
        const float hl = l.specular * s;
        diff = diff + hl;
    }
    const float lit = diff * att;
    const float e = lit * l.intensity;
    const uint32_t q = f32_to_u32((e > 16.0f ? 16.0f : e) * 256.0f);  // (a NaN stays one and gives 0)
    acc[0] += mul24(q, (uint32_t)l.colour[0]), acc[1] += mul24(q, (uint32_t)l.colour[1]), acc[2] += mul24(q, (uint32_t)l.colour[2]);
}

// Steps sample and blend for a pixel with a normal: its new colour from its own colour d (both packed).
TR_HD uint32_t relight_shade(const RelightRule &q, vec3 P, vec3 n, vec3 v, uint32_t d)
{
    uint32_t s;
    if (q.flags & RELIGHT_SHOW_NORMALS) {
        const float hx = n.x * 0.5f, hy = n.y * 0.5f, hz = n.z * 0.5f;
        const float ox = hx + 0.5f, oy = hy + 0.5f, oz = hz + 0.5f;
        s = f32_to_u8(ox * 255.0f) | (f32_to_u8(oy * 255.0f) << 8) | (f32_to_u8(oz * 255.0f) << 16);
    } else {
        uint32_t acc[3] = { 0u, 0u, 0u };
        for (uint32_t l = 0; l < q.n_lights; l++) relight_light(q.lights[l], P, n, v, acc);
        s = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int c = 0; c < 3; c++) {
            const uint32_t sum = (256u * ((q.ambient >> (8 * c)) & 0xFFu) + acc[c] + 128u) >> 8;
            s |= (sum < 255u ? sum : 255u) << (8 * c);
        }
    }
    if (q.flags & RELIGHT_ALBEDO) s = layer_px<LAYER_MULTIPLY>(s, d, LAYER_FULL);
    return layer_px_by(q.mode, s, d, 255u * q.opacity);
}

// The whole rule for one pixel from its five taps.  false: it keeps its colour.
TR_HD bool relight_px(const RelightRule &q, const RelightTap &c, const RelightTap &xa, const RelightTap &xb, const RelightTap &ya,
                      const RelightTap &yb, uint32_t d, uint32_t &out)
{
    vec3 n, v;
    if (!relight_normal(q.eye, c, xa, xb, ya, yb, n, v)) return false;
    out = relight_shade(q, c.P, n, v, d);
    return true;
}

// The host's taps: every pixel's position, computed once.
struct RelightHostTaps {
    int64_t W, H;
    const float *z;
    std::vector<float> P;
    std::vector<uint8_t> ok;
    RelightHostTaps(uint32_t width, uint32_t height, const float *depth, const float *u) : W(width), H(height), z(depth), P((size_t)W * H * 3), ok((size_t)W * H)
    {
        for (int64_t y = 0; y < H; y++)
            for (int64_t x = 0; x < W; x++) {
                const size_t at = (size_t)(x + y * W);
                vec3 p = make3(0.0f, 0.0f, 0.0f);
                ok[at] = relight_position(u, (int32_t)x, (int32_t)y, z[at], p) ? 1 : 0;
                P[3 * at] = p.x, P[3 * at + 1] = p.y, P[3 * at + 2] = p.z;
            }
    }
    RelightTap operator()(int64_t x, int64_t y) const
    {
        RelightTap t;
        t.ok = false, t.P = make3(0.0f, 0.0f, 0.0f), t.z = 0.0f;
        if (x < 0 || x >= W || y < 0 || y >= H) return t;  // (whether a neighbour exists comes from its coordinates)
        const size_t at = (size_t)(x + y * W);
        t.ok = ok[at] != 0, t.P = make3(P[3 * at], P[3 * at + 1], P[3 * at + 2]), t.z = z[at];
        return t;
    }
};

// The rule over a whole frame on the host (the body of tr_relight_host; the caller has checked the parameters).  rgb and
// out: W x H rgb8, row 0 = top; out may be rgb (a pixel reads its own colour and depths alone); z: index x + y * W, y up.
inline void relight_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const RelightRule &q, uint8_t *out)
{
    const int64_t W = width, H = height;
    if (out != rgb) memmove(out, rgb, (size_t)(W * H * 3));
    const RelightHostTaps at(width, height, z, q.u);
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            uint8_t *o = out + ((H - 1 - y) * W + x) * 3;
            const uint32_t d = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16);
            uint32_t v = 0u;
            if (!relight_px(q, at(x, y), at(x + 1, y), at(x - 1, y), at(x, y + 1), at(x, y - 1), d, v)) continue;
            o[0] = (uint8_t)(v & 0xFFu), o[1] = (uint8_t)((v >> 8) & 0xFFu), o[2] = (uint8_t)((v >> 16) & 0xFFu);
        }
}

// Step normal alone over a whole frame (the body of tr_relight_normals_host): normals, 3 floats a pixel, and valid, a
// byte a pixel, both at index x + y * W with y up like z; a pixel without a normal gets zeros.
inline void relight_normals_host(uint32_t width, uint32_t height, const float *z, const float *u, const float *eye, float *normals, uint8_t *valid)
{
    const int64_t W = width, H = height;
    const RelightHostTaps at(width, height, z, u);
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++) {
            const size_t i = (size_t)(x + y * W);
            vec3 n = make3(0.0f, 0.0f, 0.0f), v;
            const bool has = relight_normal(eye, at(x, y), at(x + 1, y), at(x - 1, y), at(x, y + 1), at(x, y - 1), n, v);
            valid[i] = has ? 1 : 0;
            normals[3 * i] = has ? n.x : 0.0f, normals[3 * i + 1] = has ? n.y : 0.0f, normals[3 * i + 2] = has ? n.z : 0.0f;
        }
}

// k_relight's arguments, passed by value (the light table with them: it is wave-uniform).  fb and out: rgb8, buffer row
// height - 1 - y; out is fb (in place) or does not overlap it, at any byte address.  fbclean / zclean: the frame's per-tile
// colour and z fast-clear flags over its 128 x 16 tile grid.  z: the frame's depth, y up.  lower: null, or fbclean again
// -- in place a flagged tile that is stored whole has its flag lowered.
struct RelightArgs {
    const uint8_t *fb;
    const uint32_t *fbclean;
    uint8_t *out;
    uint32_t *lower;
    const float *z;
    const uint32_t *zclean;
    DevFrame frame;
    RelightRule rule;
};

}  // namespace tr
