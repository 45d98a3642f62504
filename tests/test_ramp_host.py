"""The depth-ramp rule on the host: tr_ramp_host and tr_ramp_positions against tests/ramp_cases.py's numpy restatement of
the header's text, the rule's facts, the refusals with their full texts, the table builders, and the conditions of the
GPU cases asserted on the oracle's frames of those very cases.

Everything here needs no GPU.  tests/test_ramp.py compares the device with tr_ramp_host."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import ramp_cases as RC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, Hh = 37, 23            # the frame of the small cases
Z0 = np.float32(0.25)


@pytest.fixture(scope="module")
def T(built):
    import tiny_renderer_amd as T
    return T


def frame_and_depth(seed=1):
    """A random frame and a depth with drawn and undrawn pixels: a disc is drawn with depths in [0, 1), and the first
    drawn pixels of its rows carry the special values NaN, +inf, -inf, -0.0 and exactly Z0."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (Hh, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:Hh, 0:W]
    disc = (xx - 16) ** 2 + (yy - 11) ** 2 < 90
    z = np.where(disc, rng.random((Hh, W), np.float32), RC.F32_MIN).astype(np.float32)
    special = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(-0.0), Z0]
    for k, v in enumerate(special):
        row = 6 + 2 * k
        z[row, np.flatnonzero(disc[row])[0]] = v
    return rgb, z


def scales(n):
    """Both signs: the disc's depths [0, 1) around Z0 reach below 0, inside the table and past pmax."""
    s = np.float32((n - 1) * 256 / 0.5)
    return (s, -s)


def test_entry_points_declared_exported_and_typed(T):
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    for word in ("} tr_ramp_params;", "#define TR_RAMP_MAX_N 1024", "#define TR_RAMP_REPEAT 0x1u", "#define TR_ABI_VERSION 3",
                 "int tr_scene_set_ramp(tr_scene *s, uint32_t n, const uint8_t *rgba /* 4*n, host */);",
                 "int tr_scene_ramp(tr_scene *s, const tr_ramp_params *p, void *out /* or NULL */);",
                 "int tr_scene_get_ramped(tr_scene *s, const tr_ramp_params *p, uint8_t *rgb);",
                 "int tr_ramp_positions(const tr_ramp_params *p, uint32_t n, uint32_t count, const float *z, uint32_t *positions);",
                 "int tr_scene_debug_ramp_grid(tr_scene *s, uint32_t cap);"):
        assert word in header, word
    raw = C.CDLL(_lib.library_path())
    sigs = {"tr_scene_set_ramp": [C.c_void_p, C.c_uint32, C.c_void_p], "tr_scene_ramp": [C.c_void_p] * 3, "tr_scene_get_ramped": [C.c_void_p] * 3,
            "tr_ramp_host": [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
            "tr_ramp_positions": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p], "tr_scene_debug_ramp_grid": [C.c_void_p, C.c_uint32]}
    for name, args in sigs.items():
        assert hasattr(raw, name), name + " is not exported"
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
    assert C.sizeof(T.RampParams) == 32
    assert T.load_library().tr_abi_version() == 3
    src = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "tr_scene.cpp")).read()
    assert "sizeof(tr_ramp_params) == 32" in src and '"k_ramp"' in src
    for name in ("ramp_host", "ramp_positions", "ramp_params", "RampParams", "ramp_span", "ramp_span_auto", "ramp_fog", "ramp_grey", "ramp_false_colour",
                 "ramp_contours", "ramp_slice"):
        assert hasattr(T, name) and name in T.__all__, name
    for name in ("set_ramp", "ramp", "get_ramped", "debug_ramp_grid"):
        assert callable(getattr(T.Scene, name)), name


@pytest.mark.parametrize("n", RC.NS)
@pytest.mark.parametrize("mode", RC.MODES)
def test_host_rule_equals_the_numpy_rule_in_every_byte(T, mode, n):
    """Seven modes x four table sizes x {clamp, REPEAT} x both signs of scale x five opacities x undrawn alpha 0, 130 and
    255; the conditions that show the cases reach what they are for are asserted."""
    rgb, z = frame_and_depth()
    tab = RC.random_table(np.random.default_rng(7 + n), n)
    pmax = (n - 1) * 256
    keep_rgb, keep_z, keep_tab = rgb.copy(), z.copy(), tab.copy()
    drawn = RC.bits(z) != RC.F32_MIN_BITS
    assert drawn.any() and not drawn.all()
    assert np.isnan(z).any() and (z == np.inf).any() and (z == -np.inf).any() and (RC.bits(z) == 0x80000000).any() and (RC.bits(z) == RC.bits(Z0)).any()
    for scale in scales(n):
        p, _ = RC.positions_np(z, Z0, scale, n)
        assert (p[drawn] == 0).any() and (p[drawn] == pmax).any() and ((p[drawn] > 0) & (p[drawn] < pmax) & (p[drawn] & 255 != 0)).any()
        for repeat in (False, True):
            for k, opacity in enumerate(RC.OPACITIES):
                und = RC.undrawn_of((0, 130, 255)[k % 3])
                params = T.ramp_params(Z0, scale, mode, opacity, und, repeat)
                want = RC.rule_np(rgb, z, tab, Z0, scale, mode, opacity, und, repeat)
                got = T.ramp_host(rgb, z, tab, params)
                what = "scale %r repeat %r opacity %d" % (float(scale), repeat, opacity)
                assert np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))
                assert np.array_equal(T.ramp_host(rgb, z, tab, params, in_place=True), want), "in place, " + what
                if opacity == 0:
                    assert np.array_equal(got, rgb)
    assert np.array_equal(rgb, keep_rgb) and np.array_equal(RC.bits(z), RC.bits(keep_z)) and np.array_equal(tab, keep_tab)


def test_the_facts_of_the_rule(T):
    rgb, z = frame_and_depth(3)
    rng = np.random.default_rng(11)
    n = 17
    scale = scales(n)[1]
    drawn = (RC.bits(z) != RC.F32_MIN_BITS)[::-1]
    tab = RC.random_table(rng, n)
    for mode in RC.MODES:
        # cov == 0 is the identity: opacity 0, or alpha 0 in the table and in `undrawn`
        assert np.array_equal(T.ramp_host(rgb, z, tab, T.ramp_params(Z0, scale, mode, 0, RC.undrawn_of(255))), rgb), mode
        clear = tab.copy()
        clear[:, 3] = 0
        assert np.array_equal(T.ramp_host(rgb, z, clear, T.ramp_params(Z0, scale, mode, 256, RC.undrawn_of(0))), rgb), mode
        # a constant table: no dependence on z
        const = np.tile(np.array([[90, 14, 201, 177]], np.uint8), (n, 1))
        a = T.ramp_host(rgb, z, const, T.ramp_params(Z0, scale, mode, 211, (90, 14, 201, 177)))
        zz = np.where(RC.bits(z) != RC.F32_MIN_BITS, np.float32(0.9) - z, z).astype(np.float32)
        assert np.array_equal(a, T.ramp_host(rgb, zz, const, T.ramp_params(Z0, -scale, mode, 211, (90, 14, 201, 177), True))), mode
    # cov == 65280 under NORMAL: the entry's colour exactly -- a depth view
    opaque = tab.copy()
    opaque[:, 3] = 255
    view = T.ramp_host(rgb, z, opaque, T.ramp_params(Z0, scale, undrawn=(1, 2, 3, 255)))
    p, _ = RC.positions_np(z, Z0, scale, n)
    want = np.where(drawn[..., None], RC.entries_np(opaque, p)[::-1][..., :3], np.array((1, 2, 3))).astype(np.uint8)
    assert np.array_equal(view, want)
    # p == pmax gives the last entry, p == 0 the first
    flat = np.full((Hh, W), Z0, np.float32)
    assert (T.ramp_host(rgb, flat, opaque, T.ramp_params(Z0, scale)) == opaque[0, :3]).all()
    far = np.full((Hh, W), Z0 - np.float32(100.0), np.float32)
    assert (T.ramp_positions(T.ramp_params(Z0, scale), n, far) == (n - 1) * 256).all()
    assert (T.ramp_host(rgb, far, opaque, T.ramp_params(Z0, scale)) == opaque[-1, :3]).all()
    # an undrawn alpha of 0 leaves the background alone, 255 under NORMAL replaces it
    out = T.ramp_host(rgb, z, opaque, T.ramp_params(Z0, scale, undrawn=RC.undrawn_of(0)))
    assert np.array_equal(out[~drawn], rgb[~drawn]) and not np.array_equal(out[drawn], rgb[drawn])
    out = T.ramp_host(rgb, z, opaque, T.ramp_params(Z0, scale, undrawn=RC.undrawn_of(255)))
    assert (out[~drawn] == RC.FOG).all()


def test_positions(T):
    rgb, z = frame_and_depth(5)
    for n in RC.NS:
        for scale in scales(n):
            for repeat in (False, True):
                got = T.ramp_positions(T.ramp_params(Z0, scale, repeat=repeat), n, z)
                p, drawn = RC.positions_np(z, Z0, scale, n, repeat)
                assert got.dtype == np.uint32 and got.shape == z.shape
                assert np.array_equal(got[drawn], p[drawn].astype(np.uint32)) and (got[~drawn] == T.RAMP_NO_POSITION).all()
                assert int(got[drawn].max()) <= (n - 1) * 256 - (1 if repeat else 0)
    # the special depths under scale > 0: NaN and -inf give 0, +inf saturates and is clamped, -0.0 and Z0 itself are exact
    q = T.ramp_params(Z0, 1000.0)
    got = T.ramp_positions(q, 256, np.array([np.nan, np.inf, -np.inf, -0.0, Z0, Z0 + np.float32(0.125), RC.F32_MIN], np.float32))
    assert got.tolist() == [0, 255 * 256, 0, 0, 0, 125, 0xFFFFFFFF]
    assert T.ramp_positions(T.ramp_params(Z0, 1000.0, repeat=True), 256, np.array([np.inf], np.float32)).tolist() == [0xFFFFFFFF % (255 * 256)]
    assert T.ramp_positions(q, 2, np.zeros((0,), np.float32)).shape == (0,)


def test_refusals_with_their_full_texts(T):
    from tiny_renderer_amd import _lib
    L = T.load_library()

    def text():
        return L.tr_last_error().decode()

    rgb, out, z = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.float32)
    tab, pos = np.zeros((2, 4), np.uint8), np.zeros(16, np.uint32)

    def params(**kw):
        f = dict(z0=0.0, scale=1.0, mode=0, opacity=256, undrawn=0, flags=0, r0=0, r1=0)
        f.update(kw)
        return T.RampParams(f["z0"], f["scale"], f["mode"], f["opacity"], f["undrawn"], f["flags"], (C.c_uint32 * 2)(f["r0"], f["r1"]))

    def host(p, n=2, rgb_=rgb, z_=z, tab_=tab, out_=out, w=4, h=4):
        ptr = [None if a is None else a.ctypes.data for a in (rgb_, z_, tab_, out_)]
        return L.tr_ramp_host(w, h, ptr[0], ptr[1], None if p is None else C.addressof(p), n, ptr[2], ptr[3])

    def positions(p, n=2, z_=z, pos_=pos, count=16):
        return L.tr_ramp_positions(None if p is None else C.addressof(p), n, count, None if z_ is None else z_.ctypes.data,
                                   None if pos_ is None else pos_.ctypes.data)

    assert host(params()) == 0 and positions(params()) == 0
    assert host(params(scale=-1.0, flags=1, mode=6, opacity=0, undrawn=0xFFFFFFFF)) == 0
    bad = ((dict(z0=float("nan")), ": z0 must be finite"), (dict(z0=float("inf")), ": z0 must be finite"),
           (dict(scale=0.0), ": scale must be finite and not 0"), (dict(scale=-0.0), ": scale must be finite and not 0"),
           (dict(scale=float("-inf")), ": scale must be finite and not 0"), (dict(scale=float("nan")), ": scale must be finite and not 0"),
           (dict(mode=7), ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"), (dict(opacity=257), ": opacity must be 0..256"),
           (dict(flags=2), ": unknown flags"), (dict(flags=0x80000001), ": unknown flags"), (dict(r0=1), ": reserved must be 0"),
           (dict(r1=5), ": reserved must be 0"))
    for who, call in (("tr_ramp_host", host), ("tr_ramp_positions", positions)):
        for kw, why in bad:
            assert call(params(**kw)) == _lib.TR_E_INVALID and text() == who + why, kw
        # the order: parameters first
        assert call(params(z0=float("nan"), scale=0.0, mode=9)) == _lib.TR_E_INVALID and text() == who + ": z0 must be finite"
        assert call(params(mode=9, flags=4), n=1) == _lib.TR_E_INVALID and text() == who + ": mode must be TR_LAYER_NORMAL .. TR_LAYER_DIFFERENCE"
        assert call(None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        for n in (0, 1, 1025):
            assert call(params(), n=n) == _lib.TR_E_INVALID and text() == who + ": the table's length n must be 2..TR_RAMP_MAX_N"
    for kw in (dict(rgb_=None), dict(z_=None), dict(tab_=None), dict(out_=None)):
        assert host(params(), **kw) == _lib.TR_E_INVALID and text() == "tr_ramp_host: null argument"
    assert host(params(), w=0) == _lib.TR_E_INVALID and text() == "tr_ramp_host: the frame's width and height must be at least 1"
    assert host(params(), h=0) == _lib.TR_E_INVALID and text() == "tr_ramp_host: the frame's width and height must be at least 1"
    for kw in (dict(z_=None), dict(pos_=None)):
        assert positions(params(), **kw) == _lib.TR_E_INVALID and text() == "tr_ramp_positions: null argument"
    assert positions(params(), z_=None, pos_=None, count=0) == 0
    q = C.addressof(params())
    assert L.tr_scene_set_ramp(None, 2, tab.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_set_ramp: null scene"
    assert L.tr_scene_ramp(None, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_ramp: null scene"
    assert L.tr_scene_get_ramped(None, q, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_ramped: null scene"
    assert L.tr_scene_debug_ramp_grid(None, 3) == _lib.TR_E_INVALID and text() == "tr_scene_debug_ramp_grid: null scene"
    # python: ValueError before anything reaches the library
    for kw in (dict(z0=float("nan")), dict(scale=0.0), dict(scale=float("inf")), dict(scale=1e39), dict(mode="overlay"), dict(opacity=257), dict(opacity=True),
               dict(opacity=1.5), dict(undrawn=(1, 2, 3)), dict(undrawn=(1, 2, 3, 256))):
        f = dict(z0=0.0, scale=1.0)
        f.update(kw)
        with pytest.raises(ValueError):
            T.ramp_params(**f)
    good = T.ramp_params(0.0, 1.0)
    for call in (lambda: T.ramp_host(rgb, z, tab, None), lambda: T.ramp_host(rgb, z, tab.astype(np.int32), good), lambda: T.ramp_host(rgb, z, np.zeros((1, 4), np.uint8), good),
                 lambda: T.ramp_host(rgb, z, np.zeros((1025, 4), np.uint8), good), lambda: T.ramp_host(rgb, z, np.zeros((4, 3), np.uint8), good),
                 lambda: T.ramp_host(rgb, z[:3], tab, good), lambda: T.ramp_positions(good, 1, z), lambda: T.ramp_positions(None, 2, z),
                 lambda: T.ramp_positions(T.layer_params(2, 2), 2, z)):
        with pytest.raises(ValueError):
            call()
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 64, 64, None, []
    for cap in (-1, 1 << 32, 2.0, True, None):
        with pytest.raises(ValueError):
            s.debug_ramp_grid(cap)
    with pytest.raises(ValueError):
        s.set_ramp(np.zeros((2, 3), np.uint8))
    with pytest.raises(ValueError):
        s.ramp(None, None, params=T.layer_params(2, 2))


def test_the_builders(T):
    # ramp_span: integer-defined through float64
    z0, scale = T.ramp_span(82.0, 42.0, 256)
    assert z0.dtype == np.float32 and scale.dtype == np.float32
    assert z0 == np.float32(82.0) and scale == np.float32(255 * 256 / -40.0) and scale < 0
    assert (z0, scale) == RC.span(256)
    z0, scale = T.ramp_span(0.1, 0.7, 3)
    assert z0 == np.float32(0.1) and scale == np.float32(512.0 / (float(np.float32(0.7)) - float(np.float32(0.1)))) and scale > 0
    assert T.ramp_positions(T.ramp_params(*T.ramp_span(82.0, 42.0, 256)), 256, np.array([90.0, 82.0, 62.0, 42.0, 10.0], np.float32)).tolist() == \
        [0, 0, 255 * 128, 255 * 256, 255 * 256]
    for call in (lambda: T.ramp_span(1.0, 1.0, 4), lambda: T.ramp_span(float("nan"), 1.0, 4), lambda: T.ramp_span(0.0, float("inf"), 4),
                 lambda: T.ramp_span(0.0, 1.0, 1), lambda: T.ramp_span(0.0, 1.0, 1025), lambda: T.ramp_span(0.0, 1e-44, 1024)):
        with pytest.raises(ValueError):
            call()
    # the linear fog: integers
    for n in (2, 3, 256, 1024):
        f = T.ramp_fog((9, 80, 200), n)
        k = np.arange(n)
        assert f.shape == (n, 4) and f.dtype == np.uint8 and (f[:, :3] == (9, 80, 200)).all()
        assert np.array_equal(f[:, 3], (2 * 255 * k + (n - 1)) // (2 * (n - 1)))
        assert f[0, 3] == 0 and f[-1, 3] == 255
    assert np.array_equal(T.ramp_fog((1, 2, 3))[:, 3], np.arange(256))
    # the exponential kinds go through libm: entry 0, monotonicity and the last entry
    for kind in ("exp", "exp2"):
        for density in (0.5, 2.0, 6.0):
            f = T.ramp_fog((9, 80, 200), 256, kind, density)
            a = f[:, 3].astype(int)
            assert f.shape == (256, 4) and (f[:, :3] == (9, 80, 200)).all()
            assert a[0] == 0 and a[-1] == 255 and (np.diff(a) >= 0).all() and len(np.unique(a)) > 50
        lin = T.ramp_fog((0, 0, 0), 256)[:, 3].astype(int)
        assert (T.ramp_fog((0, 0, 0), 256, "exp", 6.0)[:, 3].astype(int) >= lin).all(), "exp fog rises faster than the linear one"
    assert (T.ramp_fog((0, 0, 0), 256, "exp2", 0.5)[:, 3].astype(int)[1:-1] < T.ramp_fog((0, 0, 0), 256)[:, 3].astype(int)[1:-1]).all()
    g = T.ramp_grey(256)
    assert g.shape == (256, 4) and (g[:, 3] == 255).all() and np.array_equal(g[:, 0], np.arange(256)) and (g[:, 0] == g[:, 1]).all() and (g[:, 0] == g[:, 2]).all()
    assert T.ramp_grey(2).tolist() == [[0, 0, 0, 255], [255, 255, 255, 255]]
    c = T.ramp_false_colour(256)
    assert c.shape == (256, 4) and (c[:, 3] == 255).all() and len(np.unique(c[:, :3], axis=0)) == 256
    assert tuple(c[0, :3]) == (0, 0, 160) and tuple(c[-1, :3]) == (160, 0, 0) and (np.abs(np.diff(c[:, :3].astype(int), axis=0)).max(1) <= 8).all()
    assert T.ramp_false_colour(7)[:, :3].tolist() == [[0, 0, 160], [0, 0, 255], [0, 255, 255], [0, 255, 0], [255, 255, 0], [255, 0, 0], [160, 0, 0]]
    b = T.ramp_contours(64, 8, (5, 6, 7))
    assert b.shape == (64, 4) and (b[:, :3] == (5, 6, 7)).all() and np.array_equal(b[:, 3] == 255, np.arange(64) % 8 == 0) and set(b[:, 3]) == {0, 255}
    m = T.ramp_slice(32, 10, 20, (250, 0, 1))
    assert (m[:, :3] == (250, 0, 1)).all() and np.array_equal(m[:, 3] == 255, (np.arange(32) >= 10) & (np.arange(32) < 20)) and set(m[:, 3]) == {0, 255}
    for call in (lambda: T.ramp_fog((0, 0, 256)), lambda: T.ramp_fog((0, 0, 0), 1), lambda: T.ramp_fog((0, 0, 0), 256, "cubic"), lambda: T.ramp_fog((0, 0, 0), 256, "exp", 0.0),
                 lambda: T.ramp_grey(1025), lambda: T.ramp_false_colour(True), lambda: T.ramp_contours(8, 0), lambda: T.ramp_contours(8, 2, (1, 2)),
                 lambda: T.ramp_slice(8, 4, 4), lambda: T.ramp_slice(8, 0, 9), lambda: T.ramp_slice(8, -1, 3)):
        with pytest.raises(ValueError):
            call()
    # a fog over a frame: the nearest pixel keeps its colour, the farthest takes the fog's, the background stays
    rgb = np.full((1, 3, 3), 100, np.uint8)
    z = np.array([[82.0, 42.0, RC.F32_MIN]], np.float32)
    out = T.ramp_host(rgb, z, T.ramp_fog(RC.FOG), T.ramp_params(*T.ramp_span(82.0, 42.0, 256)))
    assert out[0].tolist() == [[100, 100, 100], list(RC.FOG), [100, 100, 100]]


@pytest.mark.parametrize("W,Hh", RC.SIZES, ids=["%dx%d" % s for s in RC.SIZES])
def test_the_conditions_of_the_gpu_cases(T, small_synthetic, W, Hh):
    """The oracle's frame of each GPU case under the span the GPU tests use, for every table size: pixels at p == 0,
    pixels clamped at pmax, pixels strictly inside with f != 0 -- at least a quarter of the drawn ones --, undrawn pixels,
    a tile with nothing drawn, a tile with drawn and undrawn pixels, on 384 x 48 a drawn pixel in the middle tile; and
    tr_ramp_host equals the numpy rule on that frame over the short list."""
    from oracle import oracle as O
    mesh = T.apply_instances(small_synthetic[0], RC.table(W, Hh))
    s = O.Scene(W, Hh, mesh, small_synthetic[1], "phong")
    s.clear()
    s.set_light_direction(H.light(RC.LIGHT)), s.set_camera(*H.camera(RC.CAM)), s.render()
    z, fb = s.z_f32(), s.get_frame_buffer()
    s.close()
    drawn = RC.bits(z) != RC.F32_MIN_BITS
    assert drawn.any() and not drawn.all(), "drawn and undrawn pixels"
    tiles = [drawn[j:j + 16, i:i + 128] for j in range(0, Hh, 16) for i in range(0, W, 128)]
    assert any(not t.any() for t in tiles), "a tile with nothing drawn"
    assert any(t.any() and not t.all() for t in tiles), "a tile with drawn and undrawn pixels"
    if W % 128:
        assert drawn[:, W // 128 * 128:].any(), "nothing drawn in the partial tile column"
    if (W, Hh) == (384, 48):
        assert drawn[16:32, 128:256].any(), "a drawn pixel in the middle tile"
    for n in RC.NS:
        z0, scale = RC.span(n)
        assert (z0, scale) == T.ramp_span(RC.NEAR, RC.FAR, n)
        pmax = (n - 1) * 256
        for repeat in (False, True):
            p = T.ramp_positions(T.ramp_params(z0, scale, repeat=repeat), n, z)
            want, _ = RC.positions_np(z, z0, scale, n, repeat)
            assert np.array_equal(p[drawn], want[drawn].astype(np.uint32)) and (p[~drawn] == T.RAMP_NO_POSITION).all()
        p = T.ramp_positions(T.ramp_params(z0, scale), n, z)[drawn]
        inside = (p > 0) & (p < pmax) & ((p & 255) != 0)
        assert (p == 0).any() and (p == pmax).any(), "n %d: pixels in front of the ramp and behind it" % n
        assert 4 * int(inside.sum()) >= int(drawn.sum()), "n %d: %d of %d drawn pixels lie inside with f != 0" % (n, int(inside.sum()), int(drawn.sum()))
    rng = np.random.default_rng(W + Hh)
    tab = RC.random_table(rng, 256)
    z0, scale = RC.span(256)
    for mode, opacity, repeat, alpha in RC.SHORT:
        und = RC.undrawn_of(alpha)
        want = RC.rule_np(fb, z, tab, z0, scale, mode, opacity, und, repeat)
        assert not np.array_equal(want, fb)
        assert np.array_equal(T.ramp_host(fb, z, tab, T.ramp_params(z0, scale, mode, opacity, und, repeat)), want), (mode, opacity, repeat, alpha)


@pytest.mark.skipif(shutil.which(os.environ.get("CXX", "g++")) is None, reason="no host C++ compiler")
def test_the_host_check_program_compiles_and_passes(tmp_path):
    """scripts/ramp_host_check.cpp, built for the host without a sanitizer (the same program is what runs under
    -fsanitize=address,undefined by hand: its header has the line)."""
    exe = str(tmp_path / "ramp_host_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           "-I" + os.path.join(REPO, "tiny_renderer_amd", "csrc"), os.path.join(REPO, "scripts", "ramp_host_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    m = re.search(r"ramp: (\d+) interpolations, (\d+) positions, (\d+) frames, 0 mismatches", done.stdout)
    assert m and int(m.group(1)) == 256 * 256 * 256 and int(m.group(2)) >= 100000 and int(m.group(3)) >= 100
