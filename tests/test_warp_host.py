"""The warp stage on the host (no GPU): tr_warp_host against the rule restated in Python integers (tests/warp_cases.py),
the rule's consequences as known answers, the refusals with their full texts, the header's words, the exported symbols
and the grid builders.  tests/test_warp.py then pins the device to tr_warp_host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import warp_cases as WC


def noise(W, Hh, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (Hh, W, 3), dtype=np.uint8)


def same(got, want, what=""):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def host(F, grid, w, h, edge="border", border=(0, 0, 0)):
    import tiny_renderer_amd as T
    g = np.asarray(grid)
    return T.warp_host(F, g, w, h, T.warp_params(edge, border, per_channel=g.ndim == 4 and g.shape[0] == 3))


def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    header = open(os.path.join(H.REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_set_warp\(tr_scene \*s, uint32_t width, uint32_t height, uint32_t n_grids, const int32_t \*grid\);", header)
    assert re.search(r"int\s+tr_scene_warp\(tr_scene \*s, const tr_warp_params \*p, void \*out\);", header)
    assert re.search(r"int\s+tr_scene_get_warped\(tr_scene \*s, const tr_warp_params \*p, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_warp_host\(uint32_t width, uint32_t height, const uint8_t \*rgb, uint32_t out_width, uint32_t out_height, "
                     r"uint32_t n_grids,\s*const int32_t \*grid, const tr_warp_params \*p, uint8_t \*out", header)
    assert re.search(r"typedef struct tr_warp_params \{\s*uint32_t edge;[^}]*uint8_t border\[3\];[^}]*uint8_t pad;[^}]*uint32_t flags;[^}]*\} tr_warp_params;", header)
    for name, v in (("TR_WARP_CELL", "16"), ("TR_WARP_BORDER", "0u"), ("TR_WARP_CLAMP", "1u"), ("TR_WARP_PER_CHANNEL", "1u")):
        assert re.search(r"#define %s %s\b" % (name, v), header), name
    assert "} tr_warp_params;" in header and "#define TR_ABI_VERSION 3" in header
    rule_h = open(os.path.join(H.REPO, "tiny_renderer_amd", "csrc", "tr_warp.h")).read()
    assert "WARP_CELL = 16" in rule_h and ">> 8" in rule_h and ">> 16" in rule_h
    raw = C.CDLL(_lib.library_path())
    three = [C.c_void_p] * 3
    for name, args in (("tr_scene_set_warp", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]), ("tr_scene_warp", three),
                       ("tr_scene_get_warped", three),
                       ("tr_warp_host", [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])):
        assert hasattr(raw, name), name + " is not exported"
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
    assert C.sizeof(T.WarpParams) == 12
    assert (T.scene.WARP_CELL, T.scene.WARP_BORDER, T.scene.WARP_CLAMP, T.scene.WARP_PER_CHANNEL, T.scene.WARP_NODE_MAX) == (16, 0, 1, 1, 1 << 22)
    L = T.load_library()
    assert L.tr_abi_version() == 3
    p = T.warp_params()
    text = lambda: L.tr_last_error().decode()
    g = np.zeros((2, 2, 2), np.int32)
    assert L.tr_scene_set_warp(None, 4, 4, 1, g.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_set_warp: null scene"
    assert L.tr_scene_warp(None, C.addressof(p), None) == _lib.TR_E_INVALID and text() == "tr_scene_warp: null scene"
    assert L.tr_scene_get_warped(None, C.addressof(p), None) == _lib.TR_E_INVALID and text() == "tr_scene_get_warped: null scene"
    for name in ("set_warp", "warp", "get_warped", "pinned_warped"):
        assert callable(getattr(T.Scene, name))


def test_the_two_restatements_agree(built):
    F = noise(23, 19, 1)
    for w, h in ((23, 19), (17, 33), (1, 1)):
        for name, g in WC.grids(23, 19, w, h).items():
            for edge, border in ((WC.BORDER, (0, 0, 0)), (WC.BORDER, WC.PAPER), (WC.CLAMP, (9, 9, 9))):
                same(WC.rule_np(F, g, w, h, edge, border), WC.rule(F, g, w, h, edge, border), "%s %dx%d" % (name, w, h))


@pytest.mark.parametrize("edge,border", [("border", (0, 0, 0)), ("border", WC.PAPER), ("clamp", (0, 0, 0))], ids=["black", "paper", "clamp"])
def test_host_rule_equals_python_integers(built, edge, border):
    """Both edge modes, one and three grids, negative and beyond-image coordinates (the random grids reach two image
    sizes past every side), and nodes at -2^22 and 2^22."""
    e = {"border": WC.BORDER, "clamp": WC.CLAMP}[edge]
    rng = np.random.default_rng(7)
    for W, Hh, w, h in ((23, 19, 23, 19), (23, 19, 17, 33), (5, 3, 40, 20), (1, 1, 16, 16), (31, 2, 1, 1)):
        F = noise(W, Hh, W * Hh)
        for name, g in WC.grids(W, Hh, w, h).items():
            same(host(F, g, w, h, edge, border), WC.rule(F, g, w, h, e, border), "%s %dx%d -> %dx%d" % (name, W, Hh, w, h))
        gh, gw = WC.grid_shape(w, h)
        for n in (1, 3):
            g = rng.integers(-2 * 256 * max(W, Hh), 3 * 256 * max(W, Hh), (n, gh, gw, 2)).astype(np.int32)
            same(host(F, g, w, h, edge, border), WC.rule(F, g, w, h, e, border), "random, %d grids" % n)
            g[:, 0, 0], g[:, -1, -1], g[:, 0, -1] = -WC.NODE_MAX, WC.NODE_MAX, (WC.NODE_MAX, -WC.NODE_MAX)
            same(host(F, g, w, h, edge, border), WC.rule(F, g, w, h, e, border), "nodes at the ends of the range, %d grids" % n)


def test_consequences_as_known_answers(built):
    import tiny_renderer_amd as T
    W, Hh = 50, 37
    F = noise(W, Hh, 3)
    ident = T.warp_grid_identity(W, Hh)
    assert np.array_equal(ident, (256 * 16 * np.stack(np.meshgrid(np.arange(5), np.arange(4))[::1], -1)).astype(np.int32))
    same(host(F, ident, W, Hh), F, "the identity grid is a copy")
    flip = WC.nodes(lambda X, Y: (W - 1 - X, Y), W, Hh)
    assert np.array_equal(flip[..., 0], 256 * (W - 1 - 16 * np.arange(5))[None, :].repeat(4, 0))
    same(host(F, flip, W, Hh), F[:, ::-1], "a horizontal flip")
    same(host(F, WC.nodes(lambda X, Y: (X, Hh - 1 - Y), W, Hh), W, Hh), F[::-1], "a vertical flip")
    same(host(F, WC.nodes(lambda X, Y: (W - 1 - Y, X), Hh, W), Hh, W), np.rot90(F), "a quarter turn")
    same(host(F, WC.nodes(lambda X, Y: (Y, Hh - 1 - X), Hh, W), Hh, W), np.rot90(F, -1), "a quarter turn the other way")
    # a translation by whole pixels: a shifted copy with border
    want = np.empty_like(F)
    want[:] = WC.PAPER
    want[4:, 7:] = F[:-4, :-7]
    same(host(F, WC.nodes(lambda X, Y: (X - 7, Y - 4), W, Hh), W, Hh, "border", WC.PAPER), want, "a translation")
    # sx = 128 X: twice the width, exact (a + b + 1) >> 1 midpoints
    wide = host(F, WC.nodes(lambda X, Y: (X / 2.0, Y), 2 * W, Hh), 2 * W, Hh, "clamp")
    same(wide[:, 0::2], F, "even columns")
    same(wide[:, 1:-1:2], ((F[:, :-1].astype(np.int32) + F[:, 1:] + 1) >> 1).astype(np.uint8), "midpoints")
    same(wide[:, -1], F[:, -1], "the last column, clamped")
    # a constant frame stays constant under CLAMP, whatever the grid
    const = np.empty((Hh, W, 3), np.uint8)
    const[:] = (7, 200, 255)
    for name, g in WC.grids(W, Hh, 61, 29).items():
        out = host(const, g, 61, 29, "clamp")
        assert (out == const[0, 0]).all(), name
    # three grids: each channel through its own
    g3 = np.stack([ident, flip, WC.nodes(lambda X, Y: (X, Hh - 1 - Y), W, Hh)])
    out = host(F, g3, W, Hh)
    same(out[..., 0], F[..., 0]), same(out[..., 1], F[:, ::-1, 1]), same(out[..., 2], F[::-1, :, 2])


def test_refusals_with_their_texts(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    text = lambda: L.tr_last_error().decode()
    F = noise(20, 10)
    out = np.full((10, 20, 3), 0xAA, np.uint8)
    g = np.ascontiguousarray(T.warp_grid_identity(20, 10))
    g3 = np.ascontiguousarray(np.stack([g, g, g]))
    p = T.warp_params()
    pc = T.warp_params(per_channel=True)

    def call(width=20, height=10, rgb=F.ctypes.data, ow=20, oh=10, n=1, grid=g.ctypes.data, params=p, o=out.ctypes.data):
        return L.tr_warp_host(width, height, rgb, ow, oh, n, grid, C.addressof(params) if params is not None else None, o)
    assert call() == 0 and np.array_equal(out, F)
    out[:] = 0xAA
    for kw, why in ((dict(params=None), "null argument"),
                    (dict(params=T.WarpParams(2, (C.c_uint8 * 3)(), 0, 0)), "edge must be TR_WARP_BORDER or TR_WARP_CLAMP"),
                    (dict(params=T.WarpParams(0, (C.c_uint8 * 3)(), 1, 0)), "pad must be 0"),
                    (dict(params=T.WarpParams(0, (C.c_uint8 * 3)(), 0, 2)), "unknown flags"),
                    (dict(grid=None), "null grid"),
                    (dict(ow=0), "width and height must be 1..8192"), (dict(oh=8193), "width and height must be 1..8192"),
                    (dict(n=2), "n_grids must be 1 or 3 (TR_WARP_PER_CHANNEL)"), (dict(n=0), "n_grids must be 1 or 3 (TR_WARP_PER_CHANNEL)"),
                    (dict(params=pc), "TR_WARP_PER_CHANNEL needs three grids and there is one"),
                    (dict(n=3, grid=g3.ctypes.data), "three grids need TR_WARP_PER_CHANNEL"),
                    (dict(width=0), "the source is empty"), (dict(rgb=None), "null argument"), (dict(o=None), "null argument"),
                    (dict(o=F.ctypes.data), "out is rgb (a pixel reads other pixels: not in place)")):
        assert call(**kw) == _lib.TR_E_INVALID and text() == "tr_warp_host: " + why, (kw, text())
    for v in (WC.NODE_MAX + 1, -WC.NODE_MAX - 1):
        bad = g.copy()
        bad[-1, -1, 1] = v
        assert call(grid=bad.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_warp_host: a node value outside [-2^22, 2^22]"
        with pytest.raises(ValueError) as e:
            T.warp_host(F, bad, 20, 10, p)
        assert str(e.value) == "tr_warp_host: a node value outside [-2^22, 2^22]"
    assert (out == 0xAA).all(), "a refused call wrote `out`"
    for args in ((g[:-1], 20, 10), (g, 40, 10), (g.astype(np.float32), 20, 10), (np.stack([g, g]), 20, 10)):
        with pytest.raises(ValueError):
            T.warp_host(F, args[0], args[1], args[2], p)
    for kw in (dict(edge="mirror"), dict(edge=2), dict(border=(0, 0)), dict(border=(0, 256, 0))):
        with pytest.raises(ValueError):
            T.warp_params(**kw)


def test_builders(built):
    import tiny_renderer_amd as T
    W, Hh = 50, 37
    F = noise(W, Hh, 11)
    assert T.warp_grid_shape(W, Hh) == (4, 5) and T.warp_grid_shape(16, 16) == (2, 2) and T.warp_grid_shape(1, 17) == (3, 2)
    same(host(F, T.warp_grid_identity(W, Hh), W, Hh), F, "identity")
    same(host(F, T.warp_grid_from_function(lambda X, Y: (W - 1 - X, Y), W, Hh), W, Hh), F[:, ::-1], "flip")
    same(host(F, T.warp_grid_rotate(90, Hh, W, W, Hh), Hh, W), np.rot90(F), "rotate 90")
    same(host(F, T.warp_grid_rotate(-90, Hh, W, W, Hh), Hh, W), np.rot90(F, -1), "rotate -90")
    same(host(F, T.warp_grid_rotate(180, W, Hh), W, Hh), F[::-1, ::-1], "rotate 180")
    same(host(F, T.warp_grid_rotate(360, W, Hh), W, Hh), F, "rotate 360")
    same(host(F, T.warp_grid_lens(0.0, 0.0, W, Hh), W, Hh), F, "a lens without distortion")
    same(host(F, T.warp_grid_homography(np.eye(3), W, Hh), W, Hh), F, "the unit homography")
    same(host(F, T.warp_grid_homography([[1, 0, 3], [0, 1, -2], [0, 0, 1]], W, Hh), W, Hh), host(F, WC.nodes(lambda X, Y: (X + 3, Y - 2), W, Hh), W, Hh))
    same(host(F, T.warp_grid_chromatic(0.0, W, Hh), W, Hh), F, "no aberration")
    # the rounding: floor(256 v + 0.5), clipped to the node range
    g = T.warp_grid_from_function(lambda X, Y: (0 * X + 1.0 / 512, 0 * X - 1.0 / 512), 16, 16)
    assert (g[..., 0] == 1).all() and (g[..., 1] == 0).all()
    g = T.warp_grid_from_function(lambda X, Y: (X * 1e9, -Y * 1e9 - 1e9), 40, 40)
    assert g.dtype == np.int32 and g.max() == WC.NODE_MAX and g.min() == -WC.NODE_MAX
    # every node in range, whatever the parameters, and accepted by the rule
    big = [T.warp_grid_rotate(33.0, 8192, 64, zoom=0.001), T.warp_grid_lens(40.0, 900.0, 8192, 8192), T.warp_grid_chromatic(1e6, 300, 200),
           T.warp_grid_homography([[1, 0, 0], [0, 1, 0], [-0.01, 0, 1]], 640, 480), T.warp_grid_rotate(7, 300, 200), T.warp_grid_lens(-0.2, 0.05, 300, 200)]
    for g in big:
        assert g.dtype == np.int32 and np.abs(g.astype(np.int64)).max() <= WC.NODE_MAX
    host(F, big[2], 300, 200), host(F, big[3], 640, 480), host(F, big[4], 300, 200, "clamp")
    assert T.warp_grid_chromatic(2.0, W, Hh).shape == (3, 4, 5, 2)
    # a 7 degree turn moves the picture: not exact, but what the rule gives for its nodes
    g = T.warp_grid_rotate(7, W, Hh)
    same(host(F, g, W, Hh), WC.rule_np(F, g, W, Hh), "rotate 7")
