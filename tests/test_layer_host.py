"""The layer rule on the host: tr_layer_host against tests/layer_cases.py's numpy restatement of the header's text, the
two division identities over their whole ranges, the rule's facts, clipping, the refusals, the layer builders.

Everything here needs no GPU.  tests/test_layer.py compares the device with tr_layer_host."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import layer_cases as LC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, Hh = 37, 23            # the frame of the small cases
RECT = (5, 4, 21, 13)     # x, y, w, h of their layer


@pytest.fixture(scope="module")
def T(built):
    import tiny_renderer_amd as T
    return T


def frame_and_depth(seed=1):
    """A random frame and a depth with drawn and undrawn pixels: a disc is drawn."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:Hh, 0:W]
    z = np.where((xx - 16) ** 2 + (yy - 11) ** 2 < 60, rng.random((Hh, W), np.float32), LC.F32_MIN).astype(np.float32)
    return rgb, z


def test_entry_points_declared_exported_and_typed(T):
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    for word in ("} tr_layer_params;", "#define TR_LAYER_DIFFERENCE 6u", "#define TR_LAYER_WHERE_UNDRAWN 0x4u", "#define TR_ABI_VERSION 3",
                 "int tr_scene_layer(tr_scene *s, const tr_layer_params *p, const void *image, void *out /* or NULL */);",
                 "int tr_scene_layer_from_scene(tr_scene *dst, const tr_layer_params *p, tr_scene *src, void *out /* or NULL */);",
                 "int tr_scene_get_layered(tr_scene *s, const tr_layer_params *p, const void *image, uint8_t *rgb);"):
        assert word in header, word
    raw = C.CDLL(_lib.library_path())
    for name in ("tr_scene_layer", "tr_scene_layer_from_scene", "tr_scene_get_layered", "tr_layer_host"):
        assert hasattr(raw, name) and name in _lib.SYMBOLS
    assert C.sizeof(T.LayerParams) == 40
    src = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "tr_scene.cpp")).read()
    assert "sizeof(tr_layer_params) == 40" in src and '"k_layer"' in src


def test_the_two_division_identities_over_their_whole_ranges():
    n = np.arange(0, 255 * 65280 + 32640 + 1, dtype=np.uint64)
    assert np.array_equal(((n >> np.uint64(8)) * np.uint64(0x8081)) >> np.uint64(23), n // np.uint64(65280))
    assert int(((n >> np.uint64(8)) * np.uint64(0x8081)).max()) < 2 ** 32, "the product fits 32 bits"
    x = np.arange(0, 65536, dtype=np.uint64)
    assert np.array_equal((x * np.uint64(0x8081)) >> np.uint64(23), x // np.uint64(255))
    assert int((x * np.uint64(0x8081)).max()) < 2 ** 32


@pytest.mark.parametrize("fmt", LC.FORMATS)
@pytest.mark.parametrize("mode", LC.MODES)
def test_host_rule_equals_the_numpy_rule_in_every_byte(T, mode, fmt):
    """All seven modes x both formats x {no flag, KEY, WHERE_DRAWN, WHERE_UNDRAWN} x five opacities; the conditions that
    show the cases reach what they are for are asserted."""
    rgb, z = frame_and_depth()
    rng = np.random.default_rng(7)
    x, y, w, h = RECT
    ch = 4 if fmt == "rgba8" else 3
    img = LC.random_layer(rng, w, h, ch, LC.KEY)
    if ch == 4:
        alpha = img[..., 3]
        assert (alpha == 0).any() and (alpha == 255).any() and ((alpha > 0) & (alpha < 255)).any()
    hit = (img[..., :3] == LC.KEY).all(-1)
    assert hit.any() and not hit.all(), "KEY hits some pixels and not all"
    drawn = (LC.bits(z) != LC.F32_MIN_BITS)[::-1][y:y + h, x:x + w]
    assert drawn.any() and not drawn.all(), "drawn and undrawn pixels inside the rectangle"
    if mode == "add":
        total = img[..., :3].astype(int) + rgb[y:y + h, x:x + w]
        assert (total > 255).any() and not (total > 255).all(), "ADD saturates somewhere and not everywhere"
    keep_rgb, keep_img = rgb.copy(), img.copy()
    for where, key in ((None, None), (None, LC.KEY), ("drawn", None), ("undrawn", None), ("undrawn", LC.KEY)):
        for opacity in LC.OPACITIES:
            kw = dict(x=x, y=y, mode=mode, opacity=opacity, where=where, key=key)
            want = LC.rule_np(rgb, img, z=z, **kw)
            got = T.layer_host(rgb, img, z=z, **kw)
            assert np.array_equal(got, want), "%r: %d bytes differ" % (kw, int((got != want).sum()))
            assert np.array_equal(T.layer_host(rgb, img, z=z, in_place=True, **kw), want), "in place %r" % (kw,)
            if opacity == 0:
                assert np.array_equal(got, rgb)
    assert np.array_equal(rgb, keep_rgb) and np.array_equal(img, keep_img)


def test_the_facts_of_the_rule(T):
    rgb, z = frame_and_depth(3)
    rng = np.random.default_rng(11)
    full = LC.random_layer(rng, W, Hh, 3)
    rgba = LC.random_layer(rng, W, Hh, 4)
    for mode in LC.MODES:
        assert np.array_equal(T.layer_host(rgb, full, mode=mode, opacity=0), rgb), "opacity 0 leaves d"
        clear = rgba.copy()
        clear[..., 3] = 0
        assert np.array_equal(T.layer_host(rgb, clear, mode=mode), rgb), "A = 0 leaves d"
        opaque = rgba.copy()
        opaque[..., 3] = 255
        b = LC.blend_np(mode, opaque[..., :3], rgb).astype(np.uint8)
        assert np.array_equal(T.layer_host(rgb, opaque, mode=mode, opacity=256), b), "A = 255 at opacity 256 gives exactly b"
        assert np.array_equal(T.layer_host(rgb, full, mode=mode), LC.blend_np(mode, full, rgb).astype(np.uint8)), "rgb8 counts as A = 255"
    assert np.array_equal(T.layer_host(rgb, full), full), "NORMAL, opaque, frame-sized at (0, 0): a copy of the layer"
    assert np.array_equal(T.layer_host(rgb, np.full((Hh, W, 3), 255, np.uint8), mode="multiply"), rgb), "MULTIPLY by 255"
    assert np.array_equal(T.layer_host(rgb, np.zeros((Hh, W, 3), np.uint8), mode="add"), rgb), "ADD of 0"
    assert not T.layer_host(rgb, rgb.copy(), mode="difference").any(), "DIFFERENCE of a frame with itself is black"
    # the two WHERE flags are complements: together they cover the rectangle once
    drawn = T.layer_host(rgb, full, where="drawn", z=z)
    undrawn = T.layer_host(rgb, full, where="undrawn", z=z)
    mask = (LC.bits(z) != LC.F32_MIN_BITS)[::-1][..., None]
    assert np.array_equal(drawn, np.where(mask, full, rgb)) and np.array_equal(undrawn, np.where(mask, rgb, full))


def test_clipping_and_stride(T):
    rgb, _ = frame_and_depth(5)
    rng = np.random.default_rng(13)
    cases = [("left", -6, 5, 15, 9), ("right", W - 4, 5, 15, 9), ("top", 9, -4, 15, 9), ("bottom", 9, Hh - 3, 15, 9),
             ("top-left", -3, -2, 10, 10), ("top-right", W - 5, -2, 10, 10), ("bottom-left", -3, Hh - 4, 10, 10), ("bottom-right", W - 5, Hh - 4, 10, 10),
             ("covers", -4, -3, W + 9, Hh + 7), ("pixel", 17, 9, 1, 1), ("pixel at the corner", W - 1, Hh - 1, 1, 1)]
    for name, x, y, w, h in cases:
        for ch in (3, 4):
            img = LC.random_layer(rng, w, h, ch)
            for mode, opacity in (("normal", 256), ("screen", 190)):
                want = LC.rule_np(rgb, img, x, y, mode, opacity)
                assert (ch, mode) != (3, "normal") or not np.array_equal(want, rgb), name
                assert np.array_equal(T.layer_host(rgb, img, x, y, mode, opacity), want), name
                assert np.array_equal(T.layer_host(rgb, img, x, y, mode, opacity, in_place=True), want), name + " in place"
    for name, x, y in (("right of it", W, 0), ("left of it", -9, 3), ("above", 3, -9), ("below", 3, Hh), ("far away", -2 ** 31, 2 ** 31 - 1)):
        img = LC.random_layer(rng, 9, 9, 3)
        assert np.array_equal(T.layer_host(rgb, img, x, y), rgb), "a layer %s changes nothing" % name
        assert np.array_equal(T.layer_host(rgb, img, x, y, in_place=True), rgb)
    # a stride larger than the row: the layer is a window of a larger image, the bytes between its rows are not looked at
    for ch in (3, 4):
        big = LC.random_layer(rng, 31, 12, ch)
        view = big[2:11, 3:20]
        assert not view.flags["C_CONTIGUOUS"]
        want = LC.rule_np(rgb, np.ascontiguousarray(view), 4, 6, "add", 222)
        assert np.array_equal(T.layer_host(rgb, view, 4, 6, "add", 222), want)


def test_refusals_name_the_entry_point(T):
    from tiny_renderer_amd import _lib
    L = T.load_library()

    def text():
        return L.tr_last_error().decode()

    rgb, img, out = np.zeros((4, 4, 3), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((4, 4, 3), np.uint8)
    z = np.zeros((4, 4), np.float32)

    def call(p, rgb_=rgb, z_=z, img_=img, out_=out, w=4, h=4):
        ptr = [None if a is None else a.ctypes.data for a in (rgb_, z_, img_, out_)]
        return L.tr_layer_host(w, h, ptr[0], ptr[1], None if p is None else C.addressof(p), ptr[2], ptr[3])

    def params(**kw):
        f = dict(mode=0, format=0, flags=0, opacity=256, x=0, y=0, width=2, height=2, stride=0)
        f.update(kw)
        return T.LayerParams(f["mode"], f["format"], f["flags"], f["opacity"], f["x"], f["y"], f["width"], f["height"], f["stride"], (C.c_uint8 * 4)(1, 2, 3, 0))

    assert call(params()) == 0
    assert call(params(format=1, flags=1)) == 0, "KEY with RGBA8 is allowed"
    assert call(params(stride=6)) == 0 and call(params(stride=7)) == 0
    bad = ((dict(mode=7), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), (dict(format=2), ": format must be TR_LAYER_RGB8 or TR_LAYER_RGBA8"),
           (dict(flags=8), ": unknown flags"), (dict(flags=6), ": TR_LAYER_WHERE_DRAWN and TR_LAYER_WHERE_UNDRAWN exclude each other"),
           (dict(opacity=257), ": opacity must be 0..256"), (dict(width=0), ": width and height must be 1..8192"),
           (dict(height=0), ": width and height must be 1..8192"), (dict(width=8193), ": width and height must be 1..8192"),
           (dict(height=8193), ": width and height must be 1..8192"), (dict(stride=5), ": stride must be 0 or at least the bytes of a row"),
           (dict(format=1, stride=7), ": stride must be 0 or at least the bytes of a row"))
    for kw, why in bad:
        assert call(params(**kw)) == _lib.TR_E_INVALID and text() == "tr_layer_host" + why, kw
    assert call(None) == _lib.TR_E_INVALID and text() == "tr_layer_host: null argument"
    for kw in (dict(rgb_=None), dict(img_=None), dict(out_=None)):
        assert call(params(), **kw) == _lib.TR_E_INVALID and text() == "tr_layer_host: null argument"
    assert call(params(flags=2), z_=None) == _lib.TR_E_INVALID and text() == "tr_layer_host: a WHERE flag needs z"
    assert call(params(), z_=None) == 0
    assert call(params(), w=0) == _lib.TR_E_INVALID and text() == "tr_layer_host: the frame's width and height must be at least 1"
    q = C.addressof(params())
    assert L.tr_scene_layer(None, q, img.ctypes.data, None) == _lib.TR_E_INVALID and text() == "tr_scene_layer: null scene"
    assert L.tr_scene_layer_from_scene(None, q, None, None) == _lib.TR_E_INVALID and text() == "tr_scene_layer_from_scene: null scene"
    assert L.tr_scene_get_layered(None, q, img.ctypes.data, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_layered: null scene"
    for kw in (dict(mode="overlay"), dict(format="bgr8"), dict(where="both"), dict(opacity=257), dict(opacity=True), dict(key=(1, 2)), dict(key=(1, 2, 256)),
               dict(stride=5), dict(x=2 ** 31)):
        with pytest.raises(ValueError):
            T.layer_params(2, 2, **kw)
    for size in ((0, 2), (2, 8193)):
        with pytest.raises(ValueError):
            T.layer_params(*size)
    with pytest.raises(ValueError):
        T.layer_host(rgb, np.zeros((2, 2), np.uint8))
    with pytest.raises(ValueError):
        T.layer_host(rgb, img, where="drawn")


def test_the_layer_builders(T):
    g = T.layer_gradient(5, 9, (10, 20, 30), (250, 20, 0))
    assert g.shape == (9, 5, 3) and g.dtype == np.uint8 and tuple(g[0, 0]) == (10, 20, 30) and tuple(g[8, 4]) == (250, 20, 0)
    assert (np.diff(g[:, 0, 0].astype(int)) > 0).all() and (g[:, :, 1] == 20).all() and (g == g[:, :1]).all()
    assert tuple(T.layer_gradient(3, 1, (1, 2, 3), (9, 9, 9))[0, 0]) == (1, 2, 3)
    v = T.layer_vignette(64, 32, 200)
    assert v.shape == (32, 64, 3) and (v[..., 0] == v[..., 1]).all() and (v[..., 0] == v[..., 2]).all()
    assert v[16, 32, 0] == 255 and v[0, 0, 0] == v[31, 63, 0] == v[0, 63, 0] and 55 <= v[0, 0, 0] <= 70 and v[0, 32, 0] > v[0, 0, 0]
    assert (T.layer_vignette(8, 8, 0) == 255).all()
    c = T.layer_checker(10, 6, 2, (200, 0, 0), (0, 0, 200))
    assert c.shape == (6, 10, 3) and tuple(c[0, 0]) == (200, 0, 0) and tuple(c[0, 2]) == (0, 0, 200) and tuple(c[2, 0]) == (0, 0, 200) and tuple(c[3, 3]) == (200, 0, 0)
    b = T.layer_letterbox(12, 10, 3, (5, 6, 7))
    assert b.shape == (10, 12, 4) and (b[:3, :, 3] == 255).all() and (b[7:, :, 3] == 255).all() and (b[3:7, :, 3] == 0).all() and (b[..., :3] == (5, 6, 7)).all()
    # a letterbox over a frame: the bars take the colour, the middle stays
    rgb, _ = frame_and_depth(9)
    boxed = T.layer_host(rgb, T.layer_letterbox(W, Hh, 4))
    assert not boxed[:4].any() and not boxed[Hh - 4:].any() and np.array_equal(boxed[4:Hh - 4], rgb[4:Hh - 4])
    for call in (lambda: T.layer_gradient(0, 4, (0, 0, 0), (1, 1, 1)), lambda: T.layer_gradient(4, 4, (0, 0, 256), (1, 1, 1)), lambda: T.layer_vignette(4, 4, 256),
                 lambda: T.layer_checker(4, 4, 0), lambda: T.layer_letterbox(4, 4, 3), lambda: T.layer_vignette(8193, 4, 1)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.skipif(shutil.which(os.environ.get("CXX", "g++")) is None, reason="no host C++ compiler")
def test_the_host_check_program_compiles_and_passes(tmp_path):
    """scripts/layer_host_check.cpp, built for the host without a sanitizer (the same program is what runs under
    -fsanitize=address,undefined by hand: its header has the line)."""
    exe = str(tmp_path / "layer_host_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           "-I" + os.path.join(REPO, "tiny_renderer_amd", "csrc"), os.path.join(REPO, "scripts", "layer_host_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    m = re.search(r"layer: (\d+) frames, (\d+) fetches, 0 mismatches", done.stdout)
    assert m and int(m.group(1)) >= 1000 and int(m.group(2)) >= 10000
