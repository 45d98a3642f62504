"""The projector on the host: tr_projector_host and tr_projector_matrix against the identities of the rule (the layer
rule under WHERE_DRAWN), hand-computed values and the numpy restatement of tests/projector_cases.py.  No GPU needed:
tests/test_projector.py compares the device with tr_projector_host byte for byte."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import projector_cases as PC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["%dx%d" % s for s in PC.HOST_SIZES]
f32 = np.float32


@pytest.fixture(scope="module")
def T(built):
    import tiny_renderer_amd as T
    return T


def same(got, want, what=""):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def cast(T, rgb, z, m, img, mode="add", opacity=256, occluder_z=None, soft=False, depth_bias=0.0, in_place=False):
    p = T.projector_params(m, img.shape[1], img.shape[0], img.shape[2], mode, opacity, occluder_z is not None, soft, depth_bias)
    return T.projector_host(rgb, z, p, img, occluder_z, in_place)


def flat_frame(W, Hh, depth=50.0, colour=100):
    return np.full((Hh, W, 3), colour, np.uint8), np.full((Hh, W), depth, np.float32)


def test_entry_points_declared_exported_and_typed(T):
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    for word in ("} tr_projector_params;", "#define TR_PROJECTOR_OCCLUDE 0x1u", "#define TR_PROJECTOR_SOFT 0x2u", "#define TR_PROJECTOR_MAX_SIDE 8192u",
                 "#define TR_ABI_VERSION 3", "int tr_scene_projector(tr_scene *s, const tr_projector_params *p, const void *image, uint32_t image_stride,",
                 "int tr_scene_get_projector(tr_scene *s, const tr_projector_params *p, const void *image, uint32_t image_stride,",
                 "int tr_projector_host(uint32_t width, uint32_t height, const uint8_t *rgb, const float *z, const tr_projector_params *p,",
                 "int tr_projector_matrix(const tr_uniforms *view, const tr_uniforms *projector, float m[16]);"):
        assert word in header, word
    raw = C.CDLL(_lib.library_path())
    assert "global: tr_*;" in open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    sigs = {"tr_scene_projector": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
            "tr_scene_get_projector": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
            "tr_projector_host": [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
            "tr_projector_matrix": [C.c_void_p] * 3}
    for name, args in sigs.items():
        assert hasattr(raw, name), name + " is not exported"
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
    assert C.sizeof(T.ProjectorParams) == 128 and T.ProjectorParams.pw.offset == 64 and T.ProjectorParams.depth_bias.offset == 88
    assert T.ProjectorParams.reserved.offset == 92
    assert T.load_library().tr_abi_version() == 3
    src = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "tr_scene.cpp")).read()
    assert "sizeof(tr_projector_params) == 128" in src
    # the profile's table of names stays as its callers expect it -- at most 32 entries (tests/test_bilateral_host.py), ending
    # with k_lines (tests/test_lines_host.py) -- so k_projector has no entry there: its launches are counted by a hook
    names = re.search(r"kKernelNames\[\] = \{([^}]*)\}", src).group(1)
    assert len(names.split(",")) == 32 and src.count('"k_lines" };') == 1 and '"k_projector"' not in names
    assert _lib.SYMBOLS["tr_scene_debug_projector_launches"] == (C.c_int, [C.c_void_p]) and hasattr(raw, "tr_scene_debug_projector_launches")
    assert "int tr_scene_debug_projector_launches(tr_scene *s);" in header and callable(T.Scene.debug_projector_launches)
    for name in ("projector_host", "projector_matrix", "projector_params", "ProjectorParams"):
        assert hasattr(T, name) and name in T.__all__, name
    for name in ("projector", "get_projector"):
        assert callable(getattr(T.Scene, name)), name


@pytest.mark.parametrize("W,Hh", PC.HOST_SIZES, ids=IDS)
@pytest.mark.parametrize("channels", [3, 4])
def test_identity_translations_and_a_scaled_matrix_equal_the_layer_rule(T, W, Hh, channels):
    """m = identity with pw x ph = W x H is tr_layer_host with WHERE_DRAWN at (0, 0) in every byte, for all seven modes;
    a whole-pixel translation is that layer at an offset -- also with part of the frame outside the image --; 2 m is m."""
    rng = np.random.default_rng(W * Hh + channels)
    rgb, z = PC.random_frame(rng, W, Hh)
    img = PC.random_image(rng, W, Hh, channels)
    keep = (rgb.copy(), z.copy(), img.copy())
    for k, mode in enumerate(PC.MODES):
        op = (256, 200, 1, 255, 128, 77, 256)[k]
        want = T.layer_host(rgb, img, 0, 0, mode, op, "drawn", z=z)
        assert not np.array_equal(want, rgb)
        same(cast(T, rgb, z, PC.identity(), img, mode, op), want, "identity " + mode)
        same(cast(T, rgb, z, 2.0 * PC.identity(), img, mode, op), want, "2 m " + mode)
        same(cast(T, rgb, z, PC.identity(), img, mode, op, in_place=True), want, "out == rgb " + mode)
        # frame pixel (x, y) samples image (x + tx, y + ty), y up: the layer's top-left pixel is on frame pixel (-tx, ty), rows from the top
        for tx, ty in ((1, 0), (0, 1), (-2, 1), (W - 1, 0), (0, -(Hh - 1)), (3, -2)):
            lay = T.layer_host(rgb, img, -tx, ty, mode, op, "drawn", z=z)
            same(cast(T, rgb, z, PC.translation(tx, ty), img, mode, op), lay, "translation %d, %d %s" % (tx, ty, mode))
            same(cast(T, rgb, z, 2.0 * PC.translation(tx, ty), img, mode, op), lay, "2 m, translation")
    # the image misses the frame
    same(cast(T, rgb, z, PC.translation(W, 0), img), rgb, "a translation past the image")
    same(cast(T, rgb, z, PC.translation(0, -Hh), img), rgb, "a translation past the image")
    assert all(np.array_equal(a, b) for a, b in zip(keep, (rgb, z, img))), "an argument changed"


def test_a_mid_pixel_translation_is_the_rounded_mean(T):
    W, Hh = 9, 4
    rng = np.random.default_rng(3)
    img = PC.random_image(rng, W, Hh, 3)
    rgb, z = flat_frame(W, Hh, colour=0)
    got = cast(T, rgb, z, PC.translation(0.5, 0.0), img, "normal")
    a, b = img[:, :-1].astype(np.int64), img[:, 1:].astype(np.int64)
    same(got[:, :-1], ((a + b + 1) >> 1).astype(np.uint8), "half a pixel in x")
    same(got[:, -1:], rgb[:, -1:], "u = W - 0.5 is outside")
    got = cast(T, rgb, z, PC.translation(0.0, 0.5), img, "normal")
    a, b = img[1:].astype(np.int64), img[:-1].astype(np.int64)     # frame row r (from the top) is y = H - 1 - r: texels y and y + 1 are rows r and r - 1
    same(got[1:], ((a + b + 1) >> 1).astype(np.uint8), "half a pixel in y")
    same(got[:1], rgb[:1], "v = H - 0.5 is outside")


def test_w_not_positive_not_finite_and_nan_coordinates_change_nothing(T):
    W, Hh = 6, 4
    rng = np.random.default_rng(4)
    rgb, z = PC.random_frame(rng, W, Hh, holes=False)
    img = PC.random_image(rng, W, Hh, 3)
    assert not np.array_equal(cast(T, rgb, z, PC.identity(), img, "normal"), rgb)
    big = float(np.finfo(np.float32).max)
    m = PC.identity()
    for w_row in ((0, 0, 0, 0.0), (0, 0, 0, -1.0), (0, 0, -1.0, 0.0), (0, 0, big, 0.0), (0, 0, big, big)):   # w = 0, < 0, -z, +inf twice
        m[3] = w_row
        same(cast(T, rgb, z, m, img, "normal"), rgb, "w row %r" % (w_row,))
    # w = inf - inf = NaN: m[3] = (big, 0, -big, big) at z = 50 gives big x + (-inf); x = 0 gives -inf
    m[3] = (big, big, -big, 0.0)
    same(cast(T, rgb, z, m, img, "normal"), rgb, "w = NaN or -inf")
    # u = NaN: X = inf - inf with w = 1
    m = PC.identity()
    m[0] = (big, big, -big, 0.0)
    got = cast(T, rgb, z, m, img, "normal")
    same(got, rgb, "u = NaN or infinite")
    # one column accepted, the others NaN: X = x where z is 50, NaN elsewhere
    z2 = z.copy()
    z2[:, 0] = np.float32("nan")          # a NaN depth is a drawn pixel; every product with it is NaN
    m = PC.identity()
    m[0, 2] = 0.0
    m[3] = (0.0, 0.0, 0.0, 1.0)
    m[1, 2] = 1.0e-30                     # v = y + 1e-30 z: NaN in column 0
    got = cast(T, rgb, z2, m, img, "normal")
    same(got[:, 0], rgb[:, 0], "v = NaN")
    same(got[:, 1:], img[:, 1:], "the other columns take the image")


def test_the_closed_upper_edge_never_reads_past_the_image(T):
    """u == pw - 1 and v == ph - 1 are accepted and sampled with ax = ay = 0: the image lies at the very end of an
    allocation's used part and a poisoned copy with other bytes behind it gives the same frame."""
    pw, ph = 7, 5
    rng = np.random.default_rng(5)
    img = PC.random_image(rng, pw, ph, 3)
    rgb, z = flat_frame(pw, ph, colour=0)
    want = cast(T, rgb, z, PC.identity(), img, "normal")
    same(want, img, "every texel, the last column and the top row included")
    n = img.size
    for poison in (0x00, 0xFF):
        block = np.full(64 + n + 64, poison, np.uint8)
        for off in (64, 63, 61):     # odd byte addresses too
            block[:] = poison
            view = block[off:off + n].reshape(ph, pw, 3)
            view[...] = img
            same(cast(T, rgb, z, PC.identity(), view, "normal"), want, "poison %#x at %d" % (poison, off))
    # the frame is wider than the image: the last accepted column is pw - 1, the next is outside
    rgb2, z2 = flat_frame(pw + 2, ph, colour=9)
    got = cast(T, rgb2, z2, PC.identity(), img, "normal")
    same(got[:, :pw], img, "inside"), same(got[:, pw:], rgb2[:, pw:], "outside")
    # a 1 x 1 image: only frame pixel (0, 0) -- the bottom-left one -- is inside
    one = np.array([[[200, 100, 50, 255]]], np.uint8)
    got = cast(T, rgb2, z2, PC.identity(), one, "normal")
    want = rgb2.copy()
    want[-1, 0] = (200, 100, 50)
    same(got, want, "1 x 1")


def test_an_odd_address_and_a_padded_stride(T):
    W, Hh = 11, 6
    rng = np.random.default_rng(6)
    rgb, z = PC.random_frame(rng, W, Hh)
    for ch in (3, 4):
        img = PC.random_image(rng, W, Hh, ch)
        want = cast(T, rgb, z, PC.identity(), img, "screen", 200)
        stride = W * ch + 5
        block = rng.integers(0, 256, 3 + stride * Hh, dtype=np.uint8)
        view = np.lib.stride_tricks.as_strided(block[3:], (Hh, W, ch), (stride, ch, 1))
        view[...] = img
        assert view.ctypes.data % 2 == 1 or block.ctypes.data % 2 == 1 or True
        same(cast(T, rgb, z, PC.identity(), view, "screen", 200), want, "stride %d" % stride)


def test_occlusion_self_bias_undrawn_and_nan_texels(T):
    W, Hh = 12, 5
    rng = np.random.default_rng(7)
    rgb, z = PC.random_frame(rng, W, Hh)
    img = PC.random_image(rng, W, Hh, 4)
    plain = cast(T, rgb, z, PC.identity(), img, "normal")
    assert not np.array_equal(plain, rgb)
    for soft in (False, True):
        same(cast(T, rgb, z, PC.identity(), img, "normal", occluder_z=z, soft=soft, depth_bias=0.0), plain, "self, bias 0: every pixel lit")
        same(cast(T, rgb, z, PC.identity(), img, "normal", occluder_z=z, soft=soft, depth_bias=-1.0), rgb, "self, bias -1: every pixel shadowed")
        far = np.full((Hh, W), PC.F32_MIN, np.float32)
        same(cast(T, rgb, z, PC.identity(), img, "normal", occluder_z=far, soft=soft), plain, "an undrawn occluder lights")
        nan = np.full((Hh, W), np.nan, np.float32)
        same(cast(T, rgb, z, PC.identity(), img, "normal", occluder_z=nan, soft=soft), plain, "a NaN occluder lights")
        near = np.full((Hh, W), 1000.0, np.float32)
        same(cast(T, rgb, z, PC.identity(), img, "normal", occluder_z=near, soft=soft), rgb, "an occluder in front shadows")
    zn = np.where(PC.bits(z) != PC.F32_MIN_BITS, np.float32("nan"), z)
    near = np.full((Hh, W), 1000.0, np.float32)
    got = cast(T, rgb, zn, PC.identity(), img, "normal", occluder_z=near)
    # a NaN pixel depth: zp is NaN, the comparison fails, the pixel is lit
    same(got, cast(T, rgb, zn, PC.identity(), img, "normal"), "a NaN pixel depth is lit")


def test_hard_occlusion_switches_at_128_and_soft_fractions_by_hand(T):
    """One row of pixels over a 2 x 2 occluder with one near texel; the hard test takes the nearest texel from ax = 128 on,
    SOFT sums the bilinear weights of the lit texels."""
    pw, ph = 2, 2
    img = np.full((ph, pw, 3), 255, np.uint8)
    occ = np.full((ph, pw), PC.F32_MIN, np.float32)
    occ[0, 1] = 1000.0                                   # texel (1, 0), y up: shadows
    W = 256
    rgb, z = flat_frame(W, 1, colour=0)
    m = np.zeros((4, 4))
    m[0, 0], m[3, 3] = 1.0 / 256.0, 1.0                  # u = x / 256: ax = x, v = 0
    hard = cast(T, rgb, z, m, img, "normal", occluder_z=occ)
    assert (hard[0, :128] == 255).all() and (hard[0, 128:] == 0).all(), "the hard form takes texel ix + 1 from ax = 128 on"
    soft = cast(T, rgb, z, m, img, "normal", occluder_z=occ, soft=True)
    ax = np.arange(W, dtype=np.int64)
    f = ((256 - ax) * 256 + 128) >> 8                    # texel (0, 0) is lit with weight (256 - ax) * 256; (1, 0) is not
    cov = (255 * 256 * f + 128) >> 8
    want = (255 * cov + 32640) // 65280
    assert np.array_equal(soft[0, :, 0], want.astype(np.uint8)) and (soft[0, :, 0] == soft[0, :, 2]).all()
    assert soft[0, 0, 0] == 255 and soft[0, 255, 0] == 1 and soft[0, 128, 0] == 128
    # all four texels weighted: u = v = x / 256 along the diagonal, texel (1, 1) near as well
    occ[1, 1] = 1000.0
    m[1, 0] = 1.0 / 256.0
    soft = cast(T, rgb, z, m, img, "normal", occluder_z=occ, soft=True)
    lit = (256 - ax) * (256 - ax) + (256 - ax) * ax      # texels (0, 0) and (0, 1)
    f = (lit + 128) >> 8
    want = (255 * ((255 * 256 * f + 128) >> 8) + 32640) // 65280
    assert np.array_equal(soft[0, :, 1], want.astype(np.uint8))


def test_projector_matrix_is_the_double_product_rounded_once(T):
    from tests import helpers as H
    for k, (W, Hh, pw, ph) in enumerate(((200, 120, 64, 64), (131, 19, 300, 200))):
        view, proj = PC.cameras(W, Hh, pw, ph, cam=0.3 + k, side=0.9)
        got = T.projector_matrix(view, proj)
        P = np.array(proj.vpmv[:], np.float64).reshape(4, 4).T     # [row, column]
        V = np.array(view.i_vpmv[:], np.float64).reshape(4, 4).T
        want = np.zeros(16, np.float32)
        for c in range(4):
            for r in range(4):
                want[4 * c + r] = np.float32(((P[r, 0] * V[0, c] + P[r, 1] * V[1, c]) + P[r, 2] * V[2, c]) + P[r, 3] * V[3, c])
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert np.abs(got - (P @ V).T.reshape(16)).max() <= 1e-3 * np.abs(got).max()
        # the frame's own camera as the projector: the identity up to rounding
        same_cam = T.projector_matrix(view, view).reshape(4, 4).T
        assert np.abs(same_cam - np.eye(4)).max() < 1e-2
    L = T.load_library()
    m = np.zeros(16, np.float32)
    assert L.tr_projector_matrix(None, C.byref(proj), m.ctypes.data) != 0 and L.tr_last_error().decode() == "tr_projector_matrix: null argument"
    assert L.tr_projector_matrix(C.byref(proj), C.byref(view), m.ctypes.data) != 0      # (kind 0 leaves i_vpmv zero)
    assert L.tr_last_error().decode() == "tr_projector_matrix: view->i_vpmv is all zeros (tr_prepare_uniforms kind 2 fills it)"


def test_every_refusal_text_and_that_a_refusal_changes_nothing(T):
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 8, 4
    rng = np.random.default_rng(8)
    rgb, z = PC.random_frame(rng, W, Hh)
    img = PC.random_image(rng, W, Hh, 3)
    out = np.full((Hh, W, 3), 0xAA, np.uint8)
    occ = np.zeros((Hh, W), np.float32)

    def params(**kw):
        p = T.projector_params(PC.identity(), W, Hh, 3)
        for k, v in kw.items():
            if k == "m0":
                p.m[0] = v
            elif k == "r8":
                p.reserved[8] = v
            else:
                setattr(p, k, v)
        return p

    def call(p, image=img, stride=W * 3, oz=None, w=W, h=Hh, src=rgb, zz=z, o=out):
        return L.tr_projector_host(w, h, None if src is None else src.ctypes.data, None if zz is None else zz.ctypes.data,
                                   None if p is None else C.addressof(p), None if image is None else image.ctypes.data, stride,
                                   None if oz is None else oz.ctypes.data, None if o is None else o.ctypes.data)

    bad = ((dict(pw=0), "pw and ph must be 1..8192"), (dict(ph=8193), "pw and ph must be 1..8192"), (dict(channels=2), "channels must be 3 or 4"),
           (dict(mode=7), "mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), (dict(flags=4), "unknown flags"),
           (dict(flags=2), "TR_PROJECTOR_SOFT needs TR_PROJECTOR_OCCLUDE"), (dict(opacity=257), "opacity must be 0..256"),
           (dict(depth_bias=float("inf")), "depth_bias must be finite"), (dict(m0=float("nan")), "every entry of m must be finite"),
           (dict(r8=1), "reserved must be 0"), (dict(flags=1), "TR_PROJECTOR_OCCLUDE needs an occluder"))
    for kw, why in bad:
        assert call(params(**kw)) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_projector_host: " + why, kw
    assert call(None) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_projector_host: null argument"
    assert call(params(), image=None) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_projector_host: null argument"
    assert call(params(), stride=W * 3 - 1) == _lib.TR_E_INVALID
    assert L.tr_last_error().decode() == "tr_projector_host: image_stride must be at least the bytes of a row"
    assert call(params(), oz=occ) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_projector_host: an occluder needs TR_PROJECTOR_OCCLUDE"
    assert call(params(), w=0) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_projector_host: the frame's width and height must be 1..32768"
    assert call(params(), h=32769) == _lib.TR_E_INVALID
    for kw in (dict(src=None), dict(zz=None), dict(o=None)):
        assert call(params(), **kw) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_projector_host: null argument"
    assert (out == 0xAA).all(), "a refused call wrote `out`"
    assert call(params()) == 0 and not (out == 0xAA).all()
    # the Python builders refuse in the library's words
    for kw, why in ((dict(pw=0), "pw and ph must be 1..8192"), (dict(channels=5), "channels must be 3 or 4"), (dict(mode="burn"), "mode must be"),
                    (dict(soft=True), "TR_PROJECTOR_SOFT needs TR_PROJECTOR_OCCLUDE"), (dict(opacity=300), "opacity must be 0..256"),
                    (dict(depth_bias=float("nan")), "depth_bias must be finite"), (dict(m=np.full(16, np.inf)), "every entry of m must be finite")):
        args = dict(m=PC.identity(), pw=W, ph=Hh)
        args.update(kw)
        with pytest.raises(ValueError, match=why):
            T.projector_params(**args)
    with pytest.raises(ValueError):
        T.projector_host(rgb, z, params(), img[:, :-1])


def random_case(rng, k):
    """A frame, an image, an occluder and a matrix with a perspective row: depths 10..90, entries that keep every product
    far from overflow."""
    W, Hh = int(rng.integers(3, 40)), int(rng.integers(2, 12))
    pw, ph, ch = int(rng.integers(1, 30)), int(rng.integers(1, 20)), (3, 4)[k % 2]
    rgb, z = PC.random_frame(rng, W, Hh)
    img = PC.random_image(rng, pw, ph, ch)
    m = np.zeros((4, 4))
    m[0] = (rng.uniform(0.3, 1.5) * pw / W, rng.uniform(-0.2, 0.2), rng.uniform(-0.02, 0.02), rng.uniform(-2.0, 2.0))
    m[1] = (rng.uniform(-0.2, 0.2), rng.uniform(0.3, 1.5) * ph / Hh, rng.uniform(-0.02, 0.02), rng.uniform(-2.0, 2.0))
    m[2] = (rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(0.5, 1.5), rng.uniform(-5.0, 5.0))
    m[3] = (rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(-0.004, 0.004), rng.uniform(0.6, 1.4))
    if k % 5 == 4:
        m[3, 3] = -0.2      # w changes sign across the frame
        m[3, 0] = 0.03
    occ = (rng.uniform(5.0, 100.0, (ph, pw))).astype(np.float32)
    occ[rng.integers(0, 5, (ph, pw)) == 0] = PC.F32_MIN
    return rgb, z, img, m * (1.0, 7.0, 0.125)[k % 3], occ


def test_the_numpy_statement_agrees_on_random_pixels(T):
    """Steps 1 to 6 in numpy, float32 operations one at a time, against tr_projector_host on a few thousand random pixels
    under every mode, both channel counts, no occluder, hard and soft.  The inputs are checked here to keep the numpy
    statement well defined (no infinity or NaN in step 1), and to reach accepted, rejected, lit and shadowed pixels."""
    rng = np.random.default_rng(2026)
    n_px = n_ok = n_lit = n_dark = n_part = 0
    for k in range(40):
        rgb, z, img, m, occ = random_case(rng, k)
        mode, op = PC.MODES[k % 7], (256, 200, 255, 31)[k % 4]
        m16 = PC.flat(m)
        for oz, soft in ((None, False), (occ, False), (occ, True)):
            bias = float(rng.uniform(-3.0, 3.0))
            want, finite = PC.rule_np(rgb, z, m16, img, mode, op, oz, soft, bias)
            assert finite.all(), "case %d: step 1 overflows in numpy" % k
            same(cast(T, rgb, z, m, img, mode, op, oz, soft, bias), want, "case %d %s soft=%r" % (k, mode, soft))
        Hh, W = z.shape
        yy, xx = np.mgrid[0:Hh, 0:W]
        ok, ix, iy, ax, ay, zp, _ = PC.at_np(m16, img.shape[1], img.shape[0], xx, yy, z)
        ok &= PC.bits(z) != PC.F32_MIN_BITS
        n_px += ok.size
        n_ok += int(ok.sum())
        hard = cast(T, rgb, z, m, img, "normal", 256, occ, False, 0.0)
        soft = cast(T, rgb, z, m, img, "normal", 256, occ, True, 0.0)
        plain = cast(T, rgb, z, m, img, "normal", 256)
        n_lit += int(((hard == plain).all(2) & (plain != rgb).any(2)).sum())
        n_dark += int(((hard == rgb).all(2) & (plain != rgb).any(2)).sum())
        n_part += int(((soft != plain).any(2) & (soft != rgb).any(2)).sum())
    assert n_px > 4000 and n_ok > 300 and n_px - n_ok > 300, (n_px, n_ok)
    assert n_lit > 100 and n_dark > 100 and n_part > 50, (n_lit, n_dark, n_part)
