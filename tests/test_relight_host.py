"""The relight rule on the host: tr_relight_host / tr_relight_normals_host (tiny_renderer_amd/csrc/tr_relight.h) against
values worked out by hand, against the layer rule, and against the rule restated in numpy (tests/relight_cases.py).
No GPU is needed; tests/test_relight.py holds the device to tr_relight_host in every byte."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import relight_cases as RC

f32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR_EYE = (0.0, 0.0, 1.0e6)


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def grey(W, Hh, v=100):
    return np.full((Hh, W, 3), v, np.uint8)


def plane(W, Hh, a, b, c):
    yy, xx = np.mgrid[0:Hh, 0:W]
    return (a * xx + b * yy + c).astype(f32)


def params(T, u=RC.IDENTITY, eye=FAR_EYE, **kw):
    kw.setdefault("mode", "normal")
    kw.setdefault("albedo", False)
    return T.relight_params(u, eye, **kw)


def test_entry_points_are_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    for name in ("tr_scene_relight", "tr_scene_get_relit", "tr_scene_debug_relight_launches", "tr_relight_host", "tr_relight_normals_host"):
        assert "int %s(" % name in header and name in _lib.SYMBOLS and getattr(L, name).restype is C.c_int, name
    assert C.sizeof(T.Light) == 64 and C.sizeof(T.RelightParams) == 128
    assert "} tr_light;" in header and "} tr_relight_params;" in header and "#define TR_RELIGHT_MAX_LIGHTS 8u" in header
    assert L.tr_abi_version() == 3
    for name in ("Scene", "relight_host", "relight_normals_host", "relight_params", "RelightParams", "Light", "light_directional", "light_point", "light_spot"):
        assert name in T.__all__, name
    assert hasattr(T.Scene, "relight") and hasattr(T.Scene, "get_relit") and hasattr(T.Scene, "debug_relight_launches")


def test_an_exact_plane_has_one_normal_and_one_level_in_every_byte(built):
    """u is the identity, so P = (x, y, z); z = 2 x - 2 y + 50 is exact in f32.  Every difference towards +x is (1, 0, 2)
    and towards +y (0, 1, -2), whichever neighbour is taken, so N = (-2, 2, 1) exactly, |N| = 3 and n = (-2/3, 2/3, 1/3)
    rounded once per component -- for the frame's edge pixels, which have one neighbour on a side, too.  One directional
    light along +z of intensity 3: diff = n.z = RN(1/3) = 0x3EAAAAAB; e = RN(RN(1/3) * 3) = 1 exactly (the product
    1.0000000298 is nearer to 1 than to 1 + 2^-23); q = 256; the sample is (256 c + 128) >> 8 = c per channel, and NORMAL
    at opacity 256 stores it: every pixel becomes the light's colour."""
    import tiny_renderer_amd as T
    W, Hh = 130, 17
    z = plane(W, Hh, 2, -2, 50)
    p = params(T)
    n, valid = T.relight_normals_host(z, p)
    assert valid.all(), "every pixel of a plane has a normal"
    third = f32(1.0) / f32(3.0)
    assert third.view(np.uint32) == 0x3EAAAAAB
    want = np.array([f32(-2.0) / f32(3.0), f32(2.0) / f32(3.0), third], f32)
    assert np.array_equal(n, np.broadcast_to(want, n.shape)), "N is not (-2, 2, 1) / 3 everywhere"
    assert f32(third * f32(3.0)) == f32(1.0)
    out = T.relight_host(grey(W, Hh), z, p, [T.light_directional((0, 0, 1), (200, 100, 50), 3.0)])
    same(out, np.broadcast_to(np.array([200, 100, 50], np.uint8), out.shape), "the plane under one light")
    # the same plane seen from behind: N.V < 0 flips the normal, and the light from +z no longer reaches it
    back = params(T, eye=(0.0, 0.0, -1.0e6))
    nb, vb = T.relight_normals_host(z, back)
    assert vb.all() and np.array_equal(nb, -n)
    same(T.relight_host(grey(W, Hh), z, back, [T.light_directional((0, 0, 1), (200, 100, 50), 3.0)]), grey(W, Hh, 0), "from behind: ambient black alone")


def test_neighbour_choice_across_a_depth_step_and_on_a_tie(built):
    """A step between columns 5 and 6: z = x left of it, 100 right of it.  Column 5 takes its left neighbour (dx =
    (1, 0, 1), N = (-1, 0, 1) / sqrt 2), column 6 its right one (dx = (1, 0, 0), N = (0, 0, 1)); taking the other side
    would give a difference of about 95 in z.  A tie takes +x and +y: z = |x - 5| + |y - 4| + 10 has equal depth
    differences on both sides of column 5 and of row 4 but opposite slopes, and at (5, 4) N = (1, 0, 1) x (0, 1, 1) =
    (-1, -1, 1); taking -x would give (1, 0, -1) x .. with the sign of the first component turned.
    (A NaN difference cannot be planted: a pixel whose depth is NaN or infinite has no position, so the depths of two
    usable pixels are finite and their difference is a number or an infinity; the comparison's NaN arm is dead code by
    the position step, which test_pixels_without_a_position_or_a_normal_keep_their_colour pins;
    scripts/relight_host_check.cpp calls relight_difference itself with NaN and infinite depths and holds it to "takes b".)"""
    import tiny_renderer_amd as T
    W, Hh = 12, 9
    yy, xx = np.mgrid[0:Hh, 0:W]
    z = np.where(xx <= 5, xx, 100).astype(f32)
    n, valid = T.relight_normals_host(z, params(T))
    assert valid.all()
    r = f32(1.0) / np.sqrt(f32(2.0))
    assert np.array_equal(n[:, 5], np.broadcast_to(np.array([-r, 0, r], f32), (Hh, 3))), n[0, 5]
    assert np.array_equal(n[:, 4], n[:, 5]) and np.array_equal(n[:, 6], np.broadcast_to(np.array([0, 0, 1], f32), (Hh, 3))), n[0, 6]
    z = (np.abs(xx - 5) + np.abs(yy - 4) + 10).astype(f32)
    n, valid = T.relight_normals_host(z, params(T))
    t = f32(1.0) / np.sqrt(f32(3.0))
    assert valid.all() and np.array_equal(n[4, 5], np.array([-t, -t, t], f32)), n[4, 5]
    assert np.array_equal(n[4, 4], np.array([t, -t, t], f32)) and np.array_equal(n[3, 5], np.array([-t, t, t], f32))


def test_pixels_without_a_position_or_a_normal_keep_their_colour(built):
    import tiny_renderer_amd as T
    rng = np.random.default_rng(1)
    lights = [T.light_directional((0, 0, 1), (255, 255, 255), 1.0)]
    amb = dict(ambient=(90, 90, 90))

    def unchanged(rgb, z, p, what):
        same(T.relight_host(rgb, z, p, lights), rgb, what)
        same(T.relight_host(rgb, z, p, lights, in_place=True), rgb, what + ", in place")
        assert not T.relight_normals_host(z, p)[1].any(), what

    # a frame of one pixel; one drawn pixel alone among pixels that are not
    unchanged(grey(1, 1), np.full((1, 1), 5.0, f32), params(T, **amb), "1 x 1")
    z = np.full((5, 7), RC.F32_MIN, f32)
    z[2, 3] = 40.0
    rgb = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    unchanged(rgb, z, params(T, **amb), "an isolated pixel")
    # w == 0 everywhere
    u = RC.IDENTITY.copy()
    u[3, 3] = 0.0
    unchanged(rgb, plane(7, 5, 1, 1, 20), params(T, u, **amb), "w == 0")
    # collinear differences: x and y both move P along the same axis
    u = RC.IDENTITY.copy()
    u[1, 1], u[0, 1] = 0.0, 1.0
    unchanged(rgb, np.full((5, 7), 20.0, f32), params(T, u, **amb), "collinear differences")
    # NaN and infinite depths: those pixels keep their colour and give their neighbours nothing
    z = plane(9, 7, 1, 0, 20)
    z[3, 4], z[2, 2], z[4, 6] = np.nan, np.inf, -np.inf          # (each inside the frame: every neighbour keeps its other side)
    rgb = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    p = params(T, **amb)
    out = T.relight_host(rgb, z, p, lights)
    n, valid = T.relight_normals_host(z, p)
    bad = ~np.isfinite(z)
    assert not valid[bad].any() and valid[~bad].all() and np.array_equal(out[::-1][bad], rgb[::-1][bad])
    want, has, finite = RC.rule_np(rgb, z, RC.flat(RC.IDENTITY), FAR_EYE, lights, (90, 90, 90), "normal", 256)
    assert np.array_equal(has, valid)
    same(out, want, "around NaN and infinite depths")
    same(T.relight_host(rgb, z, p, lights, in_place=True), out, "in place equals out of place")
    # the pixels beside the NaN took their other neighbour: the plane's normal everywhere
    assert np.array_equal(n[~bad], np.broadcast_to(n[0, 0], n[~bad].shape))


def test_identities(built):
    import tiny_renderer_amd as T
    rng = np.random.default_rng(2)
    W, Hh = 37, 21
    rgb, z = RC.random_frame(rng, W, Hh)
    u = RC.random_u(rng, W, Hh)
    eye = (0.2, -0.1, 5.0)
    valid = T.relight_normals_host(z, params(T, u, eye))[1]
    drawn = RC.bits(z) != RC.F32_MIN_BITS
    assert valid.any() and (drawn & ~valid).any() and not (valid & ~drawn).any()
    lights = RC.random_lights(rng, 2)
    A = (70, 130, 250)
    for mode in RC.MODES:
        # no lights: the ambient colour as a constant layer where the pixel has a normal
        p = params(T, u, eye, ambient=A, mode=mode, opacity=200)
        got = T.relight_host(rgb, z, p)
        layered = T.layer_host(rgb, np.broadcast_to(np.array(A, np.uint8), rgb.shape).copy(), 0, 0, mode, 200, "drawn", z=z)
        same(np.where(valid[::-1][..., None], got, 0), np.where(valid[::-1][..., None], layered, 0), "ambient alone, " + mode)
        same(np.where(valid[::-1][..., None], rgb, got), rgb, "pixels without a normal, " + mode)
        # an intensity of 0 is no light; opacity 0 changes nothing
        dark = [T.light_point((0, 0, 3), (255, 255, 255), 0.0, 0.1, 0.5, 3)]
        same(T.relight_host(rgb, z, p, dark), got, "intensity 0, " + mode)
        same(T.relight_host(rgb, z, params(T, u, eye, ambient=A, mode=mode, opacity=0), lights), rgb, "opacity 0, " + mode)
    # two lights in one call: neither light's call alone, but the sum of the statement
    p = params(T, u, eye, ambient=(3, 2, 1), mode="add", albedo=True)
    both = T.relight_host(rgb, z, p, lights)
    assert not np.array_equal(both, T.relight_host(rgb, z, p, lights[:1])) and not np.array_equal(both, T.relight_host(rgb, z, p, lights[1:]))
    want, _, finite = RC.rule_np(rgb, z, RC.flat(u), eye, lights, (3, 2, 1), "add", 256, albedo=True)
    assert finite.all()
    same(both, want, "two lights")
    # ADD | ALBEDO under a white light of level 256 doubles every channel, saturating
    flat_z = np.full((Hh, W), 30.0, f32)
    p = params(T, mode="add", albedo=True)
    out = T.relight_host(rgb, flat_z, p, [T.light_directional((0, 0, 1), (255, 255, 255), 1.0)])
    same(out, np.minimum(255, 2 * rgb.astype(np.int64)).astype(np.uint8), "d + d * 1")


def wall(W=16, Hh=3):
    """A flat wall at z = 0 under the identity: P = (x, y, 0), n = (0, 0, 1)."""
    return grey(W, Hh, 0), np.zeros((Hh, W), f32)


def sample_of(q, colour):
    return [min(255, (q * c + 128) >> 8) for c in colour]


def test_point_light_falloff_along_a_row_by_hand(built):
    """A point light 4 above pixel (2, 1) of the wall, falloff 0.04f, intensity 2, colour (100, 0, 7).  At offset k along
    the row d2 = 16 + k^2, L.z = 4 / sqrt(d2), att = 1 / (1 + 0.04f d2), e = (L.z att) 2, q = trunc(256 e).  Offset 0:
    d2 = 16, att = 1 / 1.64f = 0.60975611, q = 312; offset 3: d2 = 25, L.z = 0.8f, 0.04f * 25 rounds to 1, att = 0.5,
    e = 0.8f, q = 204.  Red is (100 q + 128) >> 8 = 122 and 80."""
    import tiny_renderer_amd as T
    rgb, z = wall()
    light = T.light_point((2, 1, 4), (100, 0, 7), 2.0, 0.04)
    out = T.relight_host(rgb, z, params(T), [light])[::-1]
    qs = []
    for k in range(14):
        d2 = f32(f32(k) * f32(k) + f32(0.0)) + f32(16.0)     # (dot3's order: (dx dx + dy dy) + dz dz with dy = 0)
        lz = f32(4.0) / np.sqrt(d2)
        att = f32(1.0) / f32(f32(1.0) + f32(f32(0.04) * d2))
        e = f32(f32(lz * att) * f32(2.0))
        qs.append(int(f32(e * f32(256.0))))
        assert list(out[1, 2 + k]) == sample_of(qs[-1], (100, 0, 7)), (k, qs[-1], out[1, 2 + k])
    assert qs[0] == 312 and qs[3] == 204 and list(out[1, 2]) == [122, 0, 9] and list(out[1, 5]) == [80, 0, 6]
    assert all(a > b for a, b in zip(qs, qs[1:])), "the level falls along the row"


def test_spot_cone_zero_ramp_and_one_by_hand(built):
    """A spot 4 above pixel (1, 1) shining straight down, cos_outer = 0.5, cone_scale = 2, no falloff: c = L.z = 4 /
    sqrt(16 + k^2).  Offset 0: c = 1, cone = min(1, 1) = 1, e = 1, q = 256.  Offset 3: c = 0.8f, ramp = (0.8f - 0.5) 2 =
    0.60000002, e = 0.8f * 0.60000002 = 0.48000002, q = 122.  Offset 7: c = 4 / sqrt 65 < 0.5, cone = 0: no light, and with
    a black ambient term the NORMAL blend stores black.  Offset 1: ramp = (0.97014248 - 0.5) 2 = 0.94028497 < 1."""
    import tiny_renderer_amd as T
    rgb, z = wall()
    light = T.light_spot((1, 1, 4), (1, 1, 0), 10.0, 60.0, (255, 255, 255), 1.0)
    assert abs(light.cos_outer - 0.5) < 1e-6 and tuple(light.dir) == (0.0, 0.0, -1.0)
    light.cos_outer, light.cone_scale = 0.5, 2.0
    out = T.relight_host(rgb, z, params(T), [light])[::-1]
    got = [int(out[1, 1 + k, 0]) for k in range(10)]
    want = []
    for k in range(10):
        c = f32(4.0) / np.sqrt(f32(f32(k * k) + f32(16.0)))
        ramp = f32(f32(c - f32(0.5)) * f32(2.0))
        cone = f32(min(max(ramp, f32(0.0)), f32(1.0)))
        q = int(f32(f32(c * cone) * f32(256.0)))
        want.append(min(255, (q * 255 + 128) >> 8))
    assert got == want, (got, want)
    assert got[0] == 255 and got[3] == (122 * 255 + 128) >> 8 and got[7] == 0 and got[9] == 0 and 0 < got[1] < 255


def test_highlight_exponents_and_saturation_by_hand(built):
    """Pixel (0, 0) of the wall with the eye far above it: v = (0, 0, 1) exactly.  A directional light L = (0.6f, 0, 0.8f):
    diff = 0.8f; h = normalize((0.6f, 0, 1.8f)), n.h = h.z = 0.94868332; squared k times it is the exponent 2^k: k = 0:
    0.94868332, k = 3: 0.65610009 (= 0.9^4 in exact arithmetic), k = 10: 3.7e-24 -- the level moves by specular * that.
    An intensity of 100 saturates at level 16: q = 4096 and the sample is min(255, 16 c)."""
    import tiny_renderer_amd as T
    rgb, z = wall(4, 3)
    eye = (0.0, 0.0, 1.0e6)
    levels = {}
    for k in (0, 3, 10):
        light = T.light_directional((0.6, 0.0, 0.8), (255, 0, 0), 0.5, 0.75, k)
        light.dir[0], light.dir[2] = 0.6, 0.8         # (as given: the builder's renormalised values differ in the last bit)
        out = T.relight_host(rgb, z, params(T, eye=eye), [light])[::-1]
        hx, hz = f32(0.6), f32(f32(0.8) + f32(1.0))
        norm = np.sqrt(f32(f32(hx * hx + f32(0.0)) + f32(hz * hz)))
        s = f32(hz / norm)
        for _ in range(k):
            s = f32(s * s)
        e = f32(f32(f32(0.8) + f32(f32(0.75) * s)) * f32(0.5))       # att = 1: diff * 1 is diff
        levels[k] = int(f32(e * f32(256.0)))
        assert int(out[0, 0, 0]) == min(255, (levels[k] * 255 + 128) >> 8), (k, levels[k], out[0, 0])
    assert levels == {0: 193, 3: 165, 10: 102}, levels
    bright = T.light_directional((0, 0, 1), (1, 2, 255), 100.0)
    out = T.relight_host(rgb, z, params(T, eye=eye), [bright])
    same(out, np.broadcast_to(np.array([16, 32, 255], np.uint8), out.shape), "saturation at level 16")
    eight = T.relight_host(rgb, z, params(T, eye=eye), [T.light_directional((0, 0, 1), (1, 2, 255), 100.0)] * 8)
    same(eight, np.broadcast_to(np.array([128, 255, 255], np.uint8), out.shape), "eight saturated lights sum in u32")


def test_show_normals_is_the_normal_map_of_relight_normals_host(built):
    import tiny_renderer_amd as T
    rng = np.random.default_rng(3)
    W, Hh = 41, 23
    rgb, z = RC.random_frame(rng, W, Hh)
    u, eye = RC.random_u(rng, W, Hh), (0.0, 0.3, 4.0)
    p = params(T, u, eye, show_normals=True)
    n, valid = T.relight_normals_host(z, p)
    assert valid.any() and np.allclose(np.sqrt((n[valid].astype(np.float64) ** 2).sum(1)), 1.0, atol=1e-6)
    with np.errstate(all="ignore"):
        want = ((n * f32(0.5) + f32(0.5)) * f32(255.0)).astype(np.int64).astype(np.uint8)
    want = np.where(valid[..., None], want, rgb[::-1])[::-1]
    lit = T.relight_host(rgb, z, p, RC.random_lights(rng, 3))
    same(lit, want, "SHOW_NORMALS ignores the lights")
    same(lit, RC.rule_np(rgb, z, RC.flat(u), eye, show_normals=True, mode="normal")[0], "the statement")


def test_recovered_normals_of_an_analytic_sphere(built):
    """A sphere cap of radius 100 around (128, 128) in a 256 x 256 depth array, u the identity: the true normal at (x, y)
    is (x - 128, y - 128, z) / 100.  Over the pixels whose four neighbours are drawn, every one HAS a normal (a
    condition), and the largest angle between the recovered and the true normal, measured with this build, is 2.3357
    degrees -- at the rim, where a one-pixel difference spans the steepest depths; the median is 0.4478 degrees.  The error
    of a one-pixel difference scales with curvature times pixel size, so the bound is that measurement doubled: it covers
    a change of rounding between compilers, not a wrong formula (a swapped cross product is 180 degrees off; a
    difference taken over the wrong pixel or with the wrong sign tilts the rim's normals by tens of degrees)."""
    import tiny_renderer_amd as T
    yy, xx = np.mgrid[0:256, 0:256]
    r2 = 100.0 ** 2 - (xx - 128.0) ** 2 - (yy - 128.0) ** 2
    z = np.where(r2 > 0, np.sqrt(np.maximum(r2, 0.0)), 0.0).astype(f32)
    z[r2 <= 0] = RC.F32_MIN
    drawn = r2 > 0
    inner = drawn & RC.shifted(drawn, 1, 0, False) & RC.shifted(drawn, -1, 0, False) & RC.shifted(drawn, 0, 1, False) & RC.shifted(drawn, 0, -1, False)
    n, valid = T.relight_normals_host(z, T.relight_params(RC.IDENTITY, FAR_EYE))
    assert inner.sum() > 30000 and valid[inner].all(), "a pixel with four drawn neighbours has no normal"
    true = np.stack([xx - 128.0, yy - 128.0, np.sqrt(np.maximum(r2, 0.0))], axis=2) / 100.0
    cosine = np.clip((n.astype(np.float64) * true).sum(2)[inner], -1.0, 1.0)
    angle = np.degrees(np.arccos(cosine))
    print("sphere normals: max %.4f degrees, median %.4f" % (angle.max(), np.median(angle)))
    assert angle.max() <= 2 * 2.3357, angle.max()


def test_refusals_name_the_call_and_change_nothing(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 9, 5
    rgb, z = RC.random_frame(np.random.default_rng(4), W, Hh)
    out = np.full((Hh, W, 3), 0xAA, np.uint8)
    nrm, val = np.full((Hh, W, 3), 7.0, f32), np.full((Hh, W), 7, np.uint8)

    def text():
        return L.tr_last_error().decode()

    def make(**kw):
        p = params(T)
        for k, v in kw.items():
            if k == "u5":
                p.u[5] = v
            elif k == "eye1":
                p.eye[1] = v
            elif k == "r0":
                p.reserved[0] = v
            elif k == "a3":
                p.ambient[3] = v
            else:
                setattr(p, k, v)
        return p

    def lamp(**kw):
        l = T.light_spot((0, 0, 3), (0, 0, 0), 10.0, 30.0, (9, 9, 9), 1.0, 0.1, 0.2, 3)
        for k, v in kw.items():
            if k == "pos2":
                l.pos[2] = v
            elif k == "dir0":
                l.dir[0] = v
            elif k == "c3":
                l.colour[3] = v
            elif k == "r1":
                l.reserved[1] = v
            else:
                setattr(l, k, v)
        return l

    def host(p, lights, n):
        table = (T.Light * max(len(lights), 1))(*lights) if lights else None
        return L.tr_relight_host(W, Hh, rgb.ctypes.data, z.ctypes.data, C.addressof(p) if p is not None else None, table, n, out.ctypes.data)

    who = "tr_relight_host"
    bad_params = ((dict(mode=7), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), (dict(flags=4), ": unknown flags"), (dict(opacity=257), ": opacity must be 0..256"),
                  (dict(u5=float("inf")), ": every entry of u must be finite"), (dict(eye1=float("nan")), ": every entry of eye must be finite"),
                  (dict(a3=1), ": the fourth byte of ambient must be 0"), (dict(r0=1), ": reserved must be 0"))
    for kw, why in bad_params:
        assert host(make(**kw), [lamp()], 1) == _lib.TR_E_INVALID and text() == who + why, kw
        assert L.tr_relight_normals_host(W, Hh, z.ctypes.data, C.addressof(make(**kw)), nrm.ctypes.data, val.ctypes.data) == _lib.TR_E_INVALID
        assert text() == "tr_relight_normals_host" + why, kw
    bad_lights = ((dict(kind=3), ": kind must be TR_LIGHT_DIRECTIONAL .. TR_LIGHT_SPOT"), (dict(pos2=float("inf")), ": every float must be finite"),
                  (dict(dir0=float("nan")), ": every float must be finite"), (dict(cos_outer=float("nan")), ": every float must be finite"),
                  (dict(intensity=-1.0), ": intensity must be >= 0"), (dict(falloff=-0.5), ": falloff must be >= 0"), (dict(specular=-0.1), ": specular must be >= 0"),
                  (dict(cone_scale=0.0), ": cone_scale must be > 0"), (dict(cone_scale=-2.0), ": cone_scale must be > 0"),
                  (dict(shininess_log2=11), ": shininess_log2 must be 0..10"), (dict(c3=1), ": the fourth byte of colour must be 0"), (dict(r1=5), ": reserved must be 0"))
    for kw, why in bad_lights:
        assert host(make(), [lamp(), lamp(**kw)], 2) == _lib.TR_E_INVALID and text() == who + ": light 1" + why, kw
    assert host(None, [lamp()], 1) == _lib.TR_E_INVALID and text() == who + ": null argument"
    assert host(make(), [], 1) == _lib.TR_E_INVALID and text() == who + ": null argument"
    assert host(make(), [lamp()] * 9, 9) == _lib.TR_E_INVALID and text() == who + ": n_lights must be 0..TR_RELIGHT_MAX_LIGHTS"
    good, one = make(), (T.Light * 1)(lamp())
    assert L.tr_relight_host(0, Hh, rgb.ctypes.data, z.ctypes.data, C.addressof(good), one, 1, out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == who + ": the frame's width and height must be 1..32768"
    assert L.tr_relight_host(W, Hh, None, z.ctypes.data, C.addressof(good), one, 1, out.ctypes.data) == _lib.TR_E_INVALID and text() == who + ": null argument"
    assert L.tr_relight_normals_host(W, Hh, None, C.addressof(good), nrm.ctypes.data, val.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_relight_normals_host: null argument"
    assert (out == 0xAA).all() and (nrm == 7.0).all() and (val == 7).all(), "a refused call wrote its output"
    # a point light's cone_scale is not looked at; the accepted call writes
    point = T.light_point((0, 0, 3))
    assert point.cone_scale == 0.0 and host(make(), [point], 1) == 0 and not (out == 0xAA).all()
    # the builders refuse in the library's words
    for call, why in ((lambda: T.light_point((0, 0, 1), falloff=-1.0), "falloff must be >= 0"), (lambda: T.light_point((0, 0, float("inf"))), "every float must be finite"),
                      (lambda: T.light_directional((0, 0, 0)), "not all 0"), (lambda: T.light_spot((0, 0, 1), (0, 0, 0), 30.0, 20.0), "inner_deg < outer_deg"),
                      (lambda: T.light_point((0, 0, 1), shininess_log2=11), "shininess_log2 must be 0..10"), (lambda: T.relight_params(RC.IDENTITY, FAR_EYE, opacity=300), "opacity must be 0..256"),
                      (lambda: T.relight_params(RC.IDENTITY, FAR_EYE, mode="burn"), "mode must be"), (lambda: T.relight_host(rgb, z, params(T), [point] * 9), "n_lights must be"),
                      (lambda: T.relight_host(rgb, z, params(T), [7]), "lights must come from")):
        with pytest.raises(ValueError, match=why):
            call()


@pytest.mark.parametrize("W,Hh", RC.HOST_SIZES, ids=["%dx%d" % s for s in RC.HOST_SIZES])
def test_the_statement_in_numpy_agrees_on_random_frames(built, W, Hh):
    """Random depths 10..90 with a quarter of the pixels not drawn, a random mild perspective, random lights of every kind,
    every mode, ALBEDO on and off: tr_relight_host equals the numpy statement on every pixel whose intermediates stayed
    finite, and those are at least 95 % of the drawn pixels."""
    import tiny_renderer_amd as T
    rng = np.random.default_rng(W * 1000 + Hh)
    rgb, z = RC.random_frame(rng, W, Hh)
    drawn = RC.bits(z) != RC.F32_MIN_BITS
    seen_normals = 0
    for k, mode in enumerate(RC.MODES):
        u, eye = RC.random_u(rng, W, Hh), [float(v) for v in rng.uniform(-1.0, 1.0, 2)] + [float(rng.uniform(3.0, 6.0))]
        lights = RC.random_lights(rng, (1, 3, 8)[k % 3])
        amb, op, alb = [int(v) for v in rng.integers(0, 64, 3)], (256, 200, 77)[k % 3], k % 2 == 1
        p = T.relight_params(u, eye, amb, mode, op, albedo=alb)
        got = T.relight_host(rgb, z, p, lights)
        want, has, finite = RC.rule_np(rgb, z, RC.flat(u), eye, lights, amb, mode, op, albedo=alb)
        assert finite[drawn].mean() >= 0.95, "the statement is defined for %.3f of the drawn pixels" % finite[drawn].mean()
        assert np.array_equal(T.relight_normals_host(z, p)[1][finite], has[finite])
        keep = finite[::-1][..., None]
        same(np.where(keep, got, 0), np.where(keep, want, 0), "%s, %d lights" % (mode, len(lights)))
        same(T.relight_host(rgb, z, p, lights, in_place=True), got, "in place, " + mode)
        seen_normals += int(has.sum())
        if W >= 128:
            assert not np.array_equal(got, rgb), "nothing changed"
    assert seen_normals > 0 or W * Hh < 32
