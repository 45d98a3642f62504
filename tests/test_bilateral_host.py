"""The bilateral stage on the host (no GPU): tr_bilateral_host against the rule restated in numpy from its text
(tests/bilateral_cases.py), the known answers that follow from the rule, planted edges under both guides, the builders
and the parameter refusals with their full texts.  tests/test_bilateral.py then pins the device to tr_bilateral_host.
Every comparison is np.array_equal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import bilateral_cases as BC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = BC.everything()


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_bilateral\(tr_scene \*s, const tr_bilateral_params \*p, void \*out /\* or NULL \*/\);", header)
    assert re.search(r"int\s+tr_scene_get_bilateral\(tr_scene \*s, const tr_bilateral_params \*p, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_bilateral_host\(uint32_t width, uint32_t height, const uint8_t \*rgb[^;]*const float \*z[^;]*uint8_t \*out[^;]*const tr_bilateral_params \*p\);", header)
    assert "#define TR_ABI_VERSION 3" in header
    raw = C.CDLL(_lib.library_path())
    for name in ("tr_scene_bilateral", "tr_scene_get_bilateral", "tr_bilateral_host"):
        assert hasattr(raw, name), name + " is not exported"
        assert name in _lib.SYMBOLS
    assert _lib.SYMBOLS["tr_scene_bilateral"] == (C.c_int, [C.c_void_p] * 3)
    assert _lib.SYMBOLS["tr_scene_get_bilateral"] == (C.c_int, [C.c_void_p] * 3)
    assert _lib.SYMBOLS["tr_bilateral_host"] == (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4)
    assert T.load_library().tr_abi_version() == 3
    for name in ("bilateral_host", "bilateral_params", "BilateralParams", "spatial_box", "spatial_gaussian", "range_gaussian", "range_step"):
        assert name in T.__all__ and hasattr(T, name), name
    assert callable(T.Scene.bilateral) and callable(T.Scene.get_bilateral)
    source = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "tr_scene.cpp")).read()
    names = re.search(r"kKernelNames\[\] = \{([^}]*)\}", source).group(1)
    assert '"k_bilateral"' in names and len(names.split(",")) <= 32
    assert "tr_bilateral.h" in open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("name", sorted(ALL))
def test_host_rule_equals_the_text(name):
    """Noise spreads the distances over the whole table; white makes every distance 0; the depths hold two sloped planes, a
    block that is not drawn, a NaN and an infinity."""
    import tiny_renderer_amd as T
    case = ALL[name]
    for W, Hh in BC.IMAGES:
        z = BC.planes(W, Hh, seed=W)
        for k, img in enumerate([BC.image("noise", W, Hh), BC.image("white", W, Hh)]):
            for edge, border in BC.EDGES:
                got = T.bilateral_host(img, BC.params(case, edge, border), z if case["guide"] == "depth" else None)
                same(got, BC.rule(img, case, edge, border, z), "%s %dx%d image %d %s %r" % (name, W, Hh, k, edge, border))


def test_the_depth_guide_meets_every_special_value():
    """The z of the rule test does hold what its docstring says, and the distances it produces cover 0, values inside the
    table and 255."""
    z = BC.planes(131, 19)
    assert np.isnan(z).sum() == 1 and np.isinf(z).sum() == 1 and (BC.bits(z) == BC.F32_MIN_BITS).sum() > 10
    d = BC.depth_distance(z[:, 1:], z[:, :-1], BC.SCALE)
    assert set(np.unique(d)) >= {0, 255} and ((d > 0) & (d < 255)).any()
    nan, inf, lo = np.float32(np.nan), np.float32(np.inf), BC.F32_MIN
    f = lambda a, b, s=1.0: int(BC.depth_distance(np.float32(a), np.float32(b), s))
    assert f(nan, -3.0) == f(-3.0, nan) == f(nan, nan, 0.0) == 255
    assert f(inf, -3.0) == f(-3.0, -inf) == f(inf, inf) == f(inf, -3.0, 0.0) == 255
    assert f(lo, -3.0) == f(-3.0, lo) == 255 and f(lo, lo) == f(lo, lo, 3.0e38) == 0 and f(lo, -3.0, 0.0) == 0
    assert f(-9.0, -10.0, 100.0) == 100 and f(-9.0, -10.0, 254.99) == 254 and f(-9.0, -10.0, 255.0) == 255


def test_known_answers():
    import tiny_renderer_amd as T
    img = BC.image("noise", 37, 23)
    z = BC.planes(37, 23)
    Wn, Tb = BC.windows(), BC.tables()
    for guide in ("colour", "depth"):
        for edge, border in BC.EDGES:
            for t in Tb.values():
                centre = np.zeros((5, 7), np.uint8)
                centre[2, 3] = 77
                p = T.bilateral_params(centre, t, guide=guide, depth_scale=BC.SCALE, edge=edge, border=border)
                same(T.bilateral_host(img, p, z), img, "a centre-only window is the identity")
            for w in Wn.values():
                p = T.bilateral_params(w, Tb["zeros"], guide=guide, depth_scale=BC.SCALE, edge=edge, border=border)
                same(T.bilateral_host(img, p, z), img, "an all-zero range table is the identity")
    # an all-255 table is the plain weighted mean, whatever the guide and the depths
    box = T.bilateral_params(Wn["3x3"], Tb["all255"], edge="clamp")
    P = np.pad(img.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    mean = sum(P[j:j + 23, i:i + 37] for j in range(3) for i in range(3))
    same(T.bilateral_host(img, box), ((2 * mean + 9) // 18).astype(np.uint8), "the 3 x 3 mean, halves up")
    deep = T.bilateral_params(Wn["3x3"], Tb["all255"], guide="depth", depth_scale=BC.SCALE, edge="clamp")
    same(T.bilateral_host(img, deep, z), T.bilateral_host(img, box), "all 255: the guide does not matter")
    # step0 under the colour guide on two-valued noise: a pixel is the mean of its equals, itself
    two = (BC.image("noise", 30, 11) & 1) * np.uint8(200)
    same(T.bilateral_host(two, T.bilateral_params(Wn["15x15"], Tb["step0"])), two, "only equal taps count")
    # a constant frame stays under CLAMP
    for c in (0, 7, 255):
        flat = np.full((9, 11, 3), c, np.uint8)
        for name, case in ALL.items():
            assert (T.bilateral_host(flat, BC.params(case, "clamp"), BC.planes(11, 9)) == c).all(), (name, c)
    empty = np.zeros((0, 5, 3), np.uint8)
    assert T.bilateral_host(empty, box).shape == (0, 5, 3)
    # z is not read under the colour guide
    same(T.bilateral_host(img, BC.params(ALL["L_step6_colour"]), None), T.bilateral_host(img, BC.params(ALL["L_step6_colour"]), z), "colour reads no z")


def test_a_planted_edge_under_the_colour_guide():
    import tiny_renderer_amd as T
    img = BC.planted_colour()
    side = (np.arange(40) >= 20)[None, :] + np.zeros((12, 1), bool)
    d = np.abs(img[:, :, None, :].astype(np.int64) - img[:, None, :, :].astype(np.int64)).max(-1)   # [y, x, x']: within a row
    assert d[:, :20, :20].max() <= 6 and d[:, 20:, 20:].max() <= 6 and d[:, :20, 20:].min() >= 114
    box = T.spatial_box(5, 5)
    kept = T.bilateral_host(img, T.bilateral_params(box, T.range_step(6), edge="clamp"))
    same(kept, BC.same_side_mean(img, side), "each output is the rounded mean of the taps on its own side")
    assert (((kept >= 57) & (kept <= 63)) | ((kept >= 177) & (kept <= 183))).all()
    assert ((kept <= 63) == ~side[..., None]).all()
    mixed = T.bilateral_host(img, T.bilateral_params(box, np.full(256, 255, np.uint8), edge="clamp"))
    near = mixed[:, 18:22]
    assert ((near > 63) & (near < 177)).any(-1).all(), "a plain mean bleeds across the edge: the test discriminates"
    far = np.concatenate([mixed[:, :18], mixed[:, 22:]], 1)
    assert (((far >= 57) & (far <= 63)) | ((far >= 177) & (far <= 183))).all()


def test_a_planted_edge_under_the_depth_guide():
    import tiny_renderer_amd as T
    img = BC.image("noise", 40, 12)
    z = np.where(np.arange(40) < 20, np.float32(-10.0), np.float32(-9.0))[None, :] + np.zeros((12, 1), np.float32)
    side = (np.arange(40) >= 20)[None, :] + np.zeros((12, 1), bool)
    box = T.spatial_box(5, 5)
    p = T.bilateral_params(box, T.range_step(6), guide="depth", depth_scale=100.0, edge="clamp")
    got = T.bilateral_host(img, p, z.astype(np.float32))
    want = BC.same_side_mean(img, side)
    same(got, want, "no mixing across the depth edge")
    plain = T.bilateral_host(img, T.bilateral_params(box, np.full(256, 255, np.uint8), edge="clamp"))
    inner = np.r_[0:18, 22:40]
    same(got[:, inner], plain[:, inner], "a full box mean within a plane")
    assert not np.array_equal(got[:, 18:22], plain[:, 18:22]), "the plain mean mixes at the edge"
    # the colour guide on the same noise does something else altogether
    assert not np.array_equal(T.bilateral_host(img, T.bilateral_params(box, T.range_step(6), edge="clamp")), got)


def test_builders():
    import tiny_renderer_amd as T
    b = T.spatial_box(5, 3)
    assert b.shape == (3, 5) and b.dtype == np.uint8 and (b == 255).all()
    g = T.spatial_gaussian(3, 2.0)
    assert g.shape == (7, 7) and g.dtype == np.uint8 and g[3, 3] == 255 and np.array_equal(g, g.T) and np.array_equal(g, g[::-1])
    assert g[3, 4] == 225 and g[0, 0] == 27, "round(255 exp(-r^2 / (2 sigma^2)))"
    assert T.spatial_gaussian(0, 1.0).tolist() == [[255]] and (T.spatial_gaussian(7, 0.5)[0] == 0).all()
    r = T.range_gaussian(10.0)
    assert r.shape == (256,) and r.dtype == np.uint8 and r[0] == 255 and r[10] == 155 and r[255] == 0 and (np.diff(r.astype(int)) <= 0).all()
    s = T.range_step(6)
    assert s.shape == (256,) and s.dtype == np.uint8 and (s[:7] == 255).all() and not s[7:].any()
    assert T.range_step(255).all() and T.range_step(0).sum() == 255
    p = T.bilateral_params(g, r, guide="depth", depth_scale=2.5, edge="border", border=(1, 2, 3))
    assert (p.struct_size, p.kw, p.kh, p.guide, p.edge, p.depth_scale) == (512, 7, 7, 1, 0, 2.5) and list(p.border) == [1, 2, 3]
    assert list(p.spatial[:49]) == g.reshape(-1).tolist() and not any(p.spatial[49:]) and list(p.range) == r.tolist()
    q = T.bilateral_params(b, s)
    assert (q.guide, q.edge, q.depth_scale) == (0, 1, 0.0), "colour and clamp are the defaults"
    for bad in (lambda: T.spatial_box(2, 3), lambda: T.spatial_box(17, 1), lambda: T.spatial_gaussian(8, 1.0), lambda: T.spatial_gaussian(2, 0.0),
                lambda: T.range_gaussian(0.0), lambda: T.range_step(256), lambda: T.range_step(-1)):
        with pytest.raises(ValueError):
            bad()


def test_struct_and_refusals():
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    P = T.BilateralParams
    assert C.sizeof(P) == 512 and (P.depth_scale.offset, P.border.offset, P.pad.offset, P.spatial.offset, P.pad2.offset, P.range.offset) == (20, 24, 27, 28, 253, 256)
    img = BC.image("noise", 8, 6)
    z = BC.planes(8, 6)
    out = np.full_like(img, 0xAA)
    text = lambda: L.tr_last_error().decode()

    def refused(p, why, rgb=img, o=out, zz=z):
        assert L.tr_bilateral_host(8, 6, None if rgb is None else rgb.ctypes.data, None if zz is None else zz.ctypes.data, None if o is None else o.ctypes.data,
                                   None if p is None else C.addressof(p)) == _lib.TR_E_INVALID
        assert text() == "tr_bilateral_host" + why
        assert (out == 0xAA).all()

    def base(**kw):
        p = BC.params(ALL["3x3_step6_depth"])
        for k, v in kw.items():
            if k.startswith("spatial"):
                p.spatial[int(k[7:])] = v
            elif k.startswith("pad2_"):
                p.pad2[int(k[5:])] = v
            else:
                setattr(p, k, v)
        return p

    refused(None, ": null argument")
    refused(base(struct_size=508), ": struct_size is not sizeof(tr_bilateral_params)")
    for kw in (dict(kw=2), dict(kh=4), dict(kw=17), dict(kh=0)):
        refused(base(**kw), ": kw and kh must be odd and 1..15")
    for kw in (dict(spatial9=1), dict(spatial224=255), dict(kw=1)):
        refused(base(**kw), ": spatial weights outside the kw x kh window")
    refused(base(**{"spatial%d" % k: 0 for k in range(9)}), ": the window is all zeros")
    refused(base(guide=2), ": guide must be TR_BILATERAL_GUIDE_COLOUR or TR_BILATERAL_GUIDE_DEPTH")
    refused(base(edge=2), ": edge must be TR_BILATERAL_BORDER or TR_BILATERAL_CLAMP")
    for bad in (-1.0, float("inf"), float("-inf"), float("nan")):
        refused(base(depth_scale=bad), ": depth_scale must be finite and >= 0")
        refused(base(depth_scale=bad, guide=0), ": depth_scale must be finite and >= 0")
    refused(base(pad=1), ": pad and pad2 must be 0")
    for k in range(3):
        refused(base(**{"pad2_%d" % k: 1}), ": pad and pad2 must be 0")
    ok = base()
    refused(ok, ": null argument", rgb=None)
    refused(ok, ": null argument", o=None)
    refused(ok, ": null argument", zz=None)
    refused(ok, ": out is rgb (the rule reads neighbours: not in place)", o=img)
    # what passes at the ends: one weight in the last place of the largest window, the largest finite scale, z == NULL under COLOUR
    w = np.zeros((15, 15), np.uint8)
    w[14, 14] = 1
    assert T.bilateral_params(w, T.range_step(3), guide="depth", depth_scale=3.4028234663852886e38).spatial[224] == 1
    assert L.tr_bilateral_host(8, 6, img.ctypes.data, None, out.ctypes.data, C.addressof(base(guide=0))) == 0
    box, step = T.spatial_box(3, 3), T.range_step(6)
    for bad, match in ((dict(spatial=np.ones((2, 3), np.uint8)), "odd"), (dict(spatial=np.ones((3, 3))), "2-D"), (dict(spatial=np.ones((3, 17), np.uint8)), "odd"),
                       (dict(spatial=np.full((3, 3), 256)), "0..255"), (dict(spatial=np.zeros((3, 3), np.uint8)), "bilateral: the window is all zeros"),
                       (dict(range_table=np.ones(255, np.uint8)), "256"), (dict(range_table=np.full(256, -1)), "256"), (dict(guide="normal"), "guide"),
                       (dict(edge="mirror"), "edge"), (dict(border=(0, 0, 256)), "border"), (dict(depth_scale=-2.0), "bilateral: depth_scale must be finite"),
                       (dict(depth_scale=float("nan")), "bilateral: depth_scale must be finite")):
        kw = dict(spatial=box, range_table=step)
        kw.update(bad)
        with pytest.raises(ValueError, match=match):
            T.bilateral_params(**kw)
    with pytest.raises(ValueError):
        T.bilateral_host(img, T.rank_params(T.footprint_rect(3, 3)))
    with pytest.raises(ValueError, match="needs z"):
        T.bilateral_host(img, ok)
    with pytest.raises(ValueError, match="z \\[H, W\\]"):
        T.bilateral_host(img, ok, z[:, :-1])
