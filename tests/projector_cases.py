"""What tests/test_projector_host.py (CPU) and tests/test_projector.py (GPU) share: the sizes, the images, the matrices,
the cameras, and the projector rule restated in numpy from the words of include/tiny_renderer.h -- float32 operations one
at a time as numpy float32 arrays, the integer steps in int64, the blend as layer_cases.blend_np."""
import numpy as np

from tests import layer_cases as LC
from tests import outline_cases as OC

F32_MIN_BITS, F32_MIN, bits = OC.F32_MIN_BITS, OC.F32_MIN, OC.bits
MODES = LC.MODES
CAM, LIGHT = OC.CAM, OC.LIGHT
# the host identities: below one tile, a partial tile column and row, two tile columns and three tile rows
HOST_SIZES = ((5, 3), (130, 17), (257, 33))
# the device: below one tile; one tile exactly; the host's; four whole tile columns; a width that is a multiple of 4 but
# not of 16 (132) and one of neither (131) -- outline_cases' sizes with their sphere placements
GPU_SIZES = ((5, 3), (128, 16), (130, 17), (257, 33), (512, 48), (132, 17), (131, 19))
IMAGES = ((1, 1), (7, 5), (64, 64), (300, 200))
f32 = np.float32


def table(W, Hh):
    """Where the spheres stand (Scene(instances=...)) for a frame size: outline_cases' placements, which leave tiles with
    nothing drawn at their own sizes; the small placement elsewhere."""
    return OC.table(W, Hh) if (W, Hh) in OC.SIZES else (OC.AT_WIDE if W >= 256 else OC.AT_SMALL)


def identity():
    return np.eye(4, dtype=np.float64)


def translation(tx, ty, tz=0.0):
    m = np.eye(4, dtype=np.float64)
    m[0, 3], m[1, 3], m[2, 3] = tx, ty, tz
    return m


def flat(m):
    """A [4, 4] matrix indexed [row, column] as the 16 column-major float32 of tr_projector_params.m."""
    return np.asarray(m, np.float64).T.reshape(16).astype(np.float32)


def random_image(rng, pw, ph, channels):
    """Every byte value is likely; the alpha plane holds 0, 255 and values between."""
    img = rng.integers(0, 256, (ph, pw, channels), dtype=np.uint8)
    if channels == 4:
        pick = rng.integers(0, 4, (ph, pw))
        img[:, :, 3] = np.where(pick == 0, 0, np.where(pick == 1, 255, img[:, :, 3]))
    return img


def random_frame(rng, W, Hh, holes=True):
    """(rgb [H, W, 3] row 0 = top, z [H, W] y up): depths 10..90, about a quarter of the pixels not drawn."""
    rgb = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    z = rng.uniform(10.0, 90.0, (Hh, W)).astype(np.float32)
    if holes:
        z[rng.integers(0, 4, (Hh, W)) == 0] = F32_MIN
    return rgb, z


def at_np(m16, pw, ph, x, y, z):
    """Steps transform, divide and position for arrays of pixels: (ok, ix, iy, ax, ay, zp, finite) -- `finite`: no
    intermediate of step 1 overflowed to infinity or is NaN, the inputs for which this statement is well defined."""
    m = np.asarray(m16, f32)
    x, y, z = x.astype(f32), y.astype(f32), z.astype(f32)
    c, finite = [], np.ones(x.shape, bool)
    with np.errstate(all="ignore"):
        for i in range(4):
            t0, t1, t2 = m[i] * x, m[4 + i] * y, m[8 + i] * z
            s0 = t0 + t1
            s1 = s0 + t2
            ci = s1 + m[12 + i]
            for v in (t0, t1, t2, s0, s1, ci):
                assert v.dtype == f32
                finite &= np.isfinite(v)
            c.append(ci)
        w = c[3]
        ok = (w > 0) & np.isfinite(w)
        r = f32(1.0) / np.where(ok, w, f32(1.0))
        u, v, zp = c[0] * r, c[1] * r, c[2] * r
        ok &= (u >= 0) & (u <= f32(pw - 1)) & (v >= 0) & (v <= f32(ph - 1))
        su = np.floor(np.where(ok, u, f32(0)) * f32(256.0)).astype(np.int64)
        sv = np.floor(np.where(ok, v, f32(0)) * f32(256.0)).astype(np.int64)
    return ok, su >> 8, sv >> 8, su & 255, sv & 255, zp.astype(f32), finite


def rule_np(rgb, z, m16, image, mode="add", opacity=256, occluder_z=None, soft=False, depth_bias=0.0):
    """The frame with the image cast on it: rgb [H, W, 3] row 0 = top, z [H, W] y up, image [ph, pw, 3 | 4] row 0 = top,
    occluder_z [ph, pw] y up or None.  Returns (out, finite): finite as at_np's, over the drawn pixels."""
    Hh, W = z.shape
    ph, pw, ch = image.shape
    yy, xx = np.mgrid[0:Hh, 0:W]
    ok, ix, iy, ax, ay, zp, finite = at_np(m16, pw, ph, xx, yy, z)
    drawn = bits(z) != F32_MIN_BITS
    ok &= drawn
    finite |= ~drawn                      # (a pixel that is not drawn takes no step)
    up = image[::-1].astype(np.int64)
    if ch == 3:
        up = np.concatenate([up, np.full((ph, pw, 1), 255, np.int64)], axis=2)
    wt = [(256 - ax) * (256 - ay), ax * (256 - ay), (256 - ax) * ay, ax * ay]
    tex = [(np.minimum(ix + (t & 1), pw - 1), np.minimum(iy + (t >> 1), ph - 1)) for t in range(4)]   # (clamped where the weight is 0)
    for t in range(4):
        assert not ((wt[t] != 0) & ok & ((ix + (t & 1) >= pw) | (iy + (t >> 1) >= ph))).any(), "a weighted texel outside the image"
    s = (sum(wt[t][..., None] * up[tex[t][1], tex[t][0]] for t in range(4)) + (1 << 15)) >> 16
    light = np.full(z.shape, 256, np.int64)
    if occluder_z is not None:
        zo = np.asarray(occluder_z, f32)
        with np.errstate(all="ignore"):
            zt = (zp + f32(depth_bias)).astype(f32)
            if soft:
                light = (sum(np.where(~(zt < zo[tex[t][1], tex[t][0]]), wt[t], 0) for t in range(4)) + 128) >> 8
            else:
                light = np.where(~(zt < zo[np.minimum(iy + (ay >= 128), ph - 1), np.minimum(ix + (ax >= 128), pw - 1)]), 256, 0)
    cov = ((s[..., 3] * int(opacity)) * light + 128) >> 8
    cov = np.where(ok, cov, 0)[::-1][..., None]
    e = s[::-1][..., :3]
    d = rgb.astype(np.int64)
    out = ((LC.blend_np(mode, e, d) * cov + d * (65280 - cov) + 32640) // 65280).astype(np.uint8)
    return out, finite


def cameras(W, Hh, pw, ph, cam=CAM, side=0.9, behind=False):
    """(view uniforms, projector uniforms): the frame's camera as the tests' drive() sets it, and a projector that looks
    at the model from the side -- or, behind=True, one placed so that its w = 0 plane cuts the model: part of the frame
    has w <= 0."""
    import tiny_renderer_amd as T
    from tests import helpers as H
    frm, at, up = H.camera(cam)
    st, view = T.prepare_uniforms(2, W, Hh, H.light(LIGHT), frm, at, up)
    assert st == 0
    pfrm, pat, pup = H.camera(cam + side)
    if behind:
        # the projection's w is 1 - z_cam / 5 with z_cam counted from the eye towards `from - at`: an eye 4.6 units BEHIND
        # the origin that looks away from it has w = 0 on the plane d . p = -0.4, which cuts the model
        d = np.asarray(pfrm, np.float64)
        pfrm, pat = tuple(-4.6 * d), tuple(-5.6 * d)
    st, proj = T.prepare_uniforms(0, pw, ph, H.light(LIGHT), pfrm, pat, pup)
    assert st == 0
    return view, proj
