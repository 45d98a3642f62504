"""Edge anti-aliasing on the host: tr_aa_host against the rule in numpy and against answers worked out by hand, the rule's
two divisions exhaustively, every refusal with its text, and the proof that the GPU cases of tests/test_aa.py are not
vacuous.

The rule, from the opening comment of tiny_renderer_amd/csrc/tr_aa.h, is restated in tests/aa_cases.py.  The contract is
exact, so every comparison is np.array_equal."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from tests import aa_cases as AC
from tests import helpers as H

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tr_scene_antialias", "tr_scene_get_antialiased", "tr_aa_host", "tr_aa_quotients")


def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from tiny_renderer_amd.scene import AaParams
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_antialias\(tr_scene \*s, const tr_aa_params \*p, void \*out", header)
    assert re.search(r"int\s+tr_scene_get_antialiased\(tr_scene \*s, const tr_aa_params \*p, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_aa_host\(uint32_t width, uint32_t height, const uint8_t \*rgb, uint8_t \*out", header)
    assert re.search(r"int\s+tr_aa_quotients\(uint32_t which, uint32_t n, const uint32_t \*a, const uint32_t \*b, uint32_t \*out\);", header)
    for word in ("#define TR_AA_MAX_SEARCH 8", "#define TR_AA_SHOW_BLEND 0x1u", "} tr_aa_params;", "#define TR_ABI_VERSION 3"):
        assert word in header, word
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:([^}]*?)local:", exports, re.S).group(1).replace(";", " ").split()
    raw = C.CDLL(_lib.library_path())
    for name in NAMES:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name + " is not in exports.map"
        assert hasattr(raw, name), name + " is not exported"
        assert name in _lib.SYMBOLS
    assert _lib.SYMBOLS["tr_scene_antialias"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_scene_get_antialiased"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
    assert _lib.SYMBOLS["tr_aa_host"] == (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 3)
    assert _lib.SYMBOLS["tr_aa_quotients"] == (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 3)
    for name in ("aa_host", "aa_params", "AaParams"):
        assert name in T.__all__ and hasattr(T, name), name
    assert callable(T.Scene.antialias) and callable(T.Scene.get_antialiased)
    assert C.sizeof(AaParams) == 24
    assert T.load_library().tr_abi_version() == 3 and T.load_library().tr_pipeline_count() == 7


def planted_image(W, Hh, seed):
    """Flat areas, noise, long straight edges at several slopes (also steeper than one, and along the frame's border),
    single pixels and thin lines."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:Hh, 0:W]
    img = np.zeros((Hh, W, 3), np.uint8)
    img[...] = (30, 60, 90)
    for k, (slope, colour) in enumerate(((0.0, (200, 180, 40)), (0.11, (250, 250, 250)), (0.35, (10, 200, 120)), (1.0, (90, 20, 160)),
                                         (3.0, (255, 0, 0)), (-0.2, (0, 0, 0)))):
        x0 = (k * W) // 6
        band = (xs >= x0) & (xs < x0 + W // 6 + 3) & (ys > Hh / 2 + slope * (xs - x0) - 3)
        img[band] = colour
    noisy = (xs > 2 * W // 3) & (ys < Hh // 3)
    img[noisy] = rng.integers(0, 256, (int(noisy.sum()), 3), dtype=np.uint8)
    faint = (xs < W // 4) & (ys < Hh // 4)
    img[faint] = (rng.integers(0, 6, (int(faint.sum()), 3)) + 100).astype(np.uint8)   # noise below most thresholds
    img[0, :] = (255, 255, 255)                           # an edge along the top border, one down the right
    img[:, W - 1] = (0, 255, 0)
    img[Hh // 2, 3:W // 2] = (255, 255, 0)                # a thin line
    for k in range(6):
        img[(1 + 5 * k) % Hh, (2 + 11 * k) % W] = (255, 255, 255)
    return img


@pytest.mark.parametrize("W,Hh", AC.SIZES + ((37, 23), (9, 3), (1, 7), (5, 1)))
def test_host_rule_equals_the_numpy_rule(built, W, Hh):
    import tiny_renderer_amd as T
    img = planted_image(W, Hh, W * Hh)
    keep = img.copy()
    changed = 0
    for kw in AC.gpu_params() + AC.edge_params() + [dict(contrast_min=3, contrast_rel=200, search=3, subpixel=100, show_blend=True)]:
        want = AC.rule_np(img, **kw)
        got = T.aa_host(img, T.aa_params(**kw))
        assert np.array_equal(got, want["out"]), "%r: %d bytes differ" % (kw, int((got != want["out"]).sum()))
        changed += int((got != img).sum())
    assert changed > 0 and np.array_equal(img, keep), "the argument is left alone"


def test_the_two_divisions_exhaustively(built):
    """The edge term over span 2..16 and near 1..span / 2, tq over range 1..255 and a 0..3060, against Python's //."""
    import tiny_renderer_amd as T
    L = T.load_library()
    pairs = np.array([(span, near) for span in range(2, 17) for near in range(1, span // 2 + 1)], np.uint32)
    span, near = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    out = np.zeros(len(span), np.uint32)
    assert L.tr_aa_quotients(0, len(span), span.ctypes.data, near.ctypes.data, out.ctypes.data) == 0
    want = [((int(s) - 2 * int(n)) * 128 + int(s) // 2) // int(s) for s, n in pairs]
    assert out.tolist() == want and min(want) == 0 and max(want) == 112 and all(0 <= v <= 128 for v in want)
    a, rng = (np.ascontiguousarray(v.reshape(-1), np.uint32) for v in np.meshgrid(np.arange(3061), np.arange(1, 256), indexing="ij"))
    assert len(a) == 3061 * 255
    out = np.zeros(len(a), np.uint32)
    assert L.tr_aa_quotients(1, len(a), a.ctypes.data, rng.ctypes.data, out.ctypes.data) == 0
    want = np.array([min(256, (int(x) * 256) // (12 * int(r))) for x, r in zip(a.tolist(), rng.tolist())], np.uint32)
    assert np.array_equal(out, want)
    # outside the rule's ranges, and a wrong selector
    one = np.array([1], np.uint32)
    for which, x, y in ((0, 1, 1), (0, 17, 1), (0, 6, 4), (0, 6, 0), (1, 3061, 1), (1, 5, 0), (1, 5, 256)):
        xa, ya = np.array([x], np.uint32), np.array([y], np.uint32)
        assert L.tr_aa_quotients(which, 1, xa.ctypes.data, ya.ctypes.data, one.ctypes.data) != 0
        assert L.tr_last_error() == b"tr_aa_quotients: a pair outside the rule's ranges"
    assert L.tr_aa_quotients(2, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data) != 0
    assert L.tr_aa_quotients(0, 1, None, one.ctypes.data, one.ctypes.data) != 0 and L.tr_last_error() == b"tr_aa_quotients: null argument"
    assert L.tr_aa_quotients(0, 0, None, None, None) == 0


def off_of(img, **kw):
    """What the filter found: the blend weight of every pixel, through TR_AA_SHOW_BLEND (weights below 256)."""
    import tiny_renderer_amd as T
    out = T.aa_host(img, T.aa_params(show_blend=True, **kw))
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    return out[..., 0].astype(np.int64)


def test_known_answer_a_flat_image_is_returned_unchanged(built):
    import tiny_renderer_amd as T
    img = np.full((11, 13, 3), 0, np.uint8)
    img[...] = (17, 200, 90)
    for kw in (dict(), dict(contrast_min=0, contrast_rel=0, subpixel=256)):
        assert np.array_equal(T.aa_host(img, T.aa_params(**kw)), img)
        assert not off_of(img, **kw).any()


def test_known_answer_an_isolated_bright_pixel_is_pulled_down_by_the_sub_pixel_term(built):
    """M = 255 among zeros: range 255, EH = EV = 1020 (horizontal), both walks stop at k = 1, so span 2 and near 1: the
    edge term is (0 * 128 + 1) / 2 = 0.  a = 12 * 255 = 3060, tq = min(256, 3060 * 256 / 3060) = 256, sm = 256, off_s =
    subpixel.  At 192: (255 * 64 + 0 * 192 + 128) >> 8 = 64.  Its four neighbours have a = 510, tq = 42, sm = 18,
    (18 * 18) >> 8 = 1, off_s = 192 >> 8 = 0; the diagonal ones have range 0."""
    import tiny_renderer_amd as T
    img = np.zeros((9, 9, 3), np.uint8)
    img[4, 4] = 255
    want = img.copy()
    want[4, 4] = 64
    assert np.array_equal(T.aa_host(img, T.aa_params(subpixel=192)), want)
    assert np.array_equal(T.aa_host(img, T.aa_params(subpixel=0)), img)
    off = off_of(img, subpixel=192)
    assert off[4, 4] == 192 and off.sum() == 192
    # at 256 the pixel is replaced by its black neighbour, and the neighbours above and below take 1 / 256 of it
    got = T.aa_host(img, T.aa_params(subpixel=256))
    want = np.zeros_like(img)
    want[3, 4] = want[5, 4] = (255 * 1 + 128) >> 8
    assert np.array_equal(got, want)


def stair(W=28, Hh=8, at=12, level=200):
    """Black above, grey below; left of column `at` the grey starts at row 4, from `at` on at row 3."""
    img = np.zeros((Hh, W, 3), np.uint8)
    img[4:, :at] = level
    img[3:, at:] = level
    return img


RAMP = [77, 58, 43, 30, 18, 9, 0]   # ((8 - d) * 128 + (8 + d) // 2) // (8 + d) for d = 2..8: span 8 + d, near d


def test_known_answer_a_one_pixel_stair_on_a_long_horizontal_edge_and_on_a_vertical_one(built):
    """Row 3 left of the stair is black over grey: side B, the + walk stops where the grey steps up, d = 12 - x pixels
    away, the - walk runs out at 8: span 8 + d, near d, and the end's d2 = +200 has the other sign than 2 M - mid2 =
    -200: good.  Row 3 right of the stair is grey under black: side A, the - walk stops d = x - 11 away with d2 = -200
    against 2 M - mid2 = +200: the same ramp, mirrored.  The rows on the far side of the edge (row 4 on the left, row 2 on
    the right) find an end whose sign says the edge moves AWAY from them: off 0.  subpixel = 0 leaves the edge term."""
    import tiny_renderer_amd as T
    assert RAMP == [((8 - d) * 128 + (8 + d) // 2) // (8 + d) for d in range(2, 9)]
    img = stair()
    off = off_of(img, search=8, subpixel=0)
    assert [int(off[3, 12 - d]) for d in range(2, 9)] == RAMP, "the black side"
    assert [int(off[3, 11 + d]) for d in range(2, 9)] == RAMP, "the grey side"
    assert not off[4, :11].any() and not off[2, 13:].any() and not off[3, :4].any() and not off[3, 20:].any()
    assert not off[:2].any() and not off[5:].any()
    assert np.array_equal(off, AC.rule_np(img, search=8, subpixel=0)["off"])
    # what the blend makes of it: black towards the grey below it, grey towards the black above it
    out = T.aa_host(img, T.aa_params(search=8, subpixel=0))
    assert [int(out[3, 12 - d, 0]) for d in range(2, 9)] == [(200 * w + 128) >> 8 for w in RAMP]
    assert [int(out[3, 11 + d, 1]) for d in range(2, 9)] == [(200 * (256 - w) + 128) >> 8 for w in RAMP]
    # a shorter search sees a shorter edge: span 4 + d, near d
    off4 = off_of(img, search=4, subpixel=0)
    assert [int(off4[3, 12 - d]) for d in range(2, 5)] == [((4 - d) * 128 + (4 + d) // 2) // (4 + d) for d in range(2, 5)]
    # the same picture turned: a vertical edge, W for N and E for S
    turned = np.ascontiguousarray(img.transpose(1, 0, 2))
    offt = off_of(turned, search=8, subpixel=0)
    assert [int(offt[12 - d, 3]) for d in range(2, 9)] == RAMP and [int(offt[11 + d, 3]) for d in range(2, 9)] == RAMP
    assert not offt[:11, 4].any() and not offt[13:, 2].any()
    r = AC.rule_np(turned, search=8, subpixel=0)
    assert np.array_equal(offt, r["off"]) and not r["horizontal"][r["off"] > 0].any()
    assert AC.rule_np(img, search=8, subpixel=0)["horizontal"][off > 0].all()


def test_known_answer_an_edge_that_runs_into_the_frames_border(built):
    """A straight edge with its stair 3 pixels from the right border.  The walks of the pixels at the left border leave
    the frame; the clamp repeats the border pixel, the edge goes on, both walks run out and off is 0 -- a black border
    would end the edge there (d2 = -200) and blend.  At the right border the + walk of the pixels beyond the stair runs
    into the clamp as well: the - walk alone decides."""
    W = 20
    img = stair(W=W, at=W - 3)
    off = off_of(img, search=8, subpixel=0)
    assert not off[:, :W - 3 - 8].any(), "the clamp continues the edge past the left border"
    assert [int(off[3, W - 3 - d]) for d in range(2, 9)] == RAMP
    assert int(off[3, W - 1]) == RAMP[1], "x = W - 1: the - walk stops at 3, the + walk runs out in the clamp"
    turned = np.ascontiguousarray(img.transpose(1, 0, 2))
    offt = off_of(turned, search=8, subpixel=0)
    assert not offt[:W - 3 - 8].any() and [int(offt[W - 3 - d, 3]) for d in range(2, 9)] == RAMP and int(offt[W - 1, 3]) == RAMP[1]
    # an edge ON the border row: the row above row 0 is row 0 again, so N == M there
    img = np.zeros((6, 12, 3), np.uint8)
    img[0] = 200
    r = AC.rule_np(img, subpixel=0)
    assert r["passed"][0].all() and r["side_b"][0].all() and not r["off"].any()
    assert not off_of(img, subpixel=0).any()


def test_known_answer_show_blend(built):
    import tiny_renderer_amd as T
    img = np.zeros((9, 9, 3), np.uint8)
    img[4, 4] = (255, 255, 255)
    got = T.aa_host(img, T.aa_params(subpixel=256, show_blend=True))
    want = np.zeros_like(img)
    want[4, 4] = 255                                      # off = 256 shows as min(255, off)
    want[3, 4] = want[5, 4] = want[4, 3] = want[4, 5] = 1  # (the two beside it blend with black: the picture keeps them)
    assert np.array_equal(got, want)
    img = stair()
    got = T.aa_host(img, T.aa_params(subpixel=0, show_blend=True))
    assert (got[3, 10] == RAMP[0]).all() and not got[6].any(), "a kept pixel shows as 0, whatever its colour"


def test_refusals_with_their_texts(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    rgb, out = np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)
    bad = [("struct_size", 20, "struct_size is not sizeof(tr_aa_params)"), ("struct_size", 28, "struct_size is not sizeof(tr_aa_params)"),
           ("contrast_min", 256, "contrast_min must be 0..255"), ("contrast_rel", 257, "contrast_rel must be 0..256"),
           ("search", 0, "search must be 1..TR_AA_MAX_SEARCH"), ("search", 9, "search must be 1..TR_AA_MAX_SEARCH"),
           ("subpixel", 257, "subpixel must be 0..256"), ("flags", 2, "unknown flags"), ("flags", 0x80000001, "unknown flags")]
    who = "tr_aa_host"
    for field, v, text in bad:
        q = T.aa_params()
        setattr(q, field, v)
        assert L.tr_aa_host(2, 2, rgb.ctypes.data, out.ctypes.data, C.addressof(q)) == _lib.TR_E_INVALID, (field, v)
        assert L.tr_last_error().decode() == who + ": " + text
    assert L.tr_aa_host(2, 2, rgb.ctypes.data, out.ctypes.data, None) == _lib.TR_E_INVALID and L.tr_last_error() == b"tr_aa_host: null argument"
    p = T.aa_params()
    q = C.addressof(p)
    assert L.tr_aa_host(2, 2, None, out.ctypes.data, q) == _lib.TR_E_INVALID and L.tr_last_error() == b"tr_aa_host: null argument"
    assert L.tr_aa_host(2, 2, rgb.ctypes.data, None, q) == _lib.TR_E_INVALID and L.tr_last_error() == b"tr_aa_host: null argument"
    assert L.tr_aa_host(2, 2, rgb.ctypes.data, rgb.ctypes.data, q) == _lib.TR_E_INVALID
    assert L.tr_last_error() == b"tr_aa_host: out is rgb (the rule reads neighbours: not in place)"
    for w, h in ((0, 5), (5, 0), (0, 0)):
        assert L.tr_aa_host(w, h, None, None, q) == 0
    assert L.tr_scene_antialias(None, q, None) == _lib.TR_E_INVALID and L.tr_last_error() == b"tr_scene_antialias: null scene"
    assert L.tr_scene_get_antialiased(None, q, rgb.ctypes.data) == _lib.TR_E_INVALID and L.tr_last_error() == b"tr_scene_get_antialiased: null scene"


def test_python_rejects_what_the_host_can_decide():
    import tiny_renderer_amd as T
    for kw in (dict(contrast_min=-1), dict(contrast_min=256), dict(contrast_min=1.5), dict(contrast_rel=257), dict(contrast_rel=-1),
               dict(search=0), dict(search=9), dict(search=True), dict(search=2.0), dict(subpixel=257), dict(subpixel=-1), dict(subpixel=None)):
        with pytest.raises(ValueError):
            T.aa_params(**kw)
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 64, 64, None, []
    rgb = np.zeros((4, 4, 3), np.uint8)
    for call in (lambda: s.antialias(None), lambda: s.get_antialiased({}), lambda: T.aa_host(rgb, None), lambda: T.aa_host(rgb[..., :2], T.aa_params()),
                 lambda: T.aa_host(rgb, T.outline_params())):
        with pytest.raises(ValueError):
            call()
    p = T.aa_params(contrast_min=3, contrast_rel=40, search=5, subpixel=7, show_blend=True)
    assert (p.struct_size, p.contrast_min, p.contrast_rel, p.search, p.subpixel, p.flags) == (24, 3, 40, 5, 7, 1)
    d = T.aa_params()
    assert (d.contrast_min, d.contrast_rel, d.search, d.subpixel, d.flags) == (8, 32, 8, 192, 0)


def oracle_frame(ms, W, Hh, mesh):
    from oracle import oracle as O
    s = O.Scene(W, Hh, mesh, ms[1], "phong")
    s.clear()
    s.set_light_direction(H.light(AC.LIGHT)), s.set_camera(*H.camera(AC.CAM)), s.render()
    fb, z = s.get_frame_buffer(), s.z_f32()
    s.close()
    return fb, z


@pytest.mark.parametrize("W,Hh", AC.SIZES)
def test_the_gpu_cases_are_not_vacuous(built, small_synthetic, W, Hh):
    """The oracle's frame of the GPU cases, under every parameter set of AC.gpu_params(): between 0.5 % and 40 % of the
    pixels change; horizontal and vertical edges and the sides A and B each occur on at least 32 filtered pixels; every
    distance 1..search occurs as a stopping distance and at least 8 walks run out; at least 8 pixels win by the
    sub-pixel term and 8 by the edge term; some walk reads luma across a tile border in x and some across one in y."""
    import tiny_renderer_amd as T
    fb, _ = oracle_frame(small_synthetic, W, Hh, T.apply_instance_transforms(small_synthetic[0], AC.table(W, Hh)))
    ys, xs = np.mgrid[0:Hh, 0:W]
    tile_row = (Hh - 1 - ys) // 16                        # the tile grid counts rows from the bottom
    for kw in AC.gpu_params():
        r = AC.rule_np(fb, **kw)
        search = kw.get("search", 8)
        assert np.array_equal(T.aa_host(fb, T.aa_params(**kw)), r["out"])
        p = r["passed"]
        changed = (r["out"] != fb).any(-1).mean()
        assert 0.005 <= changed <= 0.40, (kw, changed)
        assert int((p & r["horizontal"]).sum()) >= 32 and int((p & ~r["horizontal"]).sum()) >= 32, kw
        assert int((p & r["side_b"]).sum()) >= 32 and int((p & ~r["side_b"]).sum()) >= 32, kw
        for k in range(1, search + 1):
            assert (p & r["stopped_m"] & (r["dist_m"] == k)).any() or (p & r["stopped_p"] & (r["dist_p"] == k)).any(), (kw, k)
        assert int((p & ~r["stopped_m"]).sum() + (p & ~r["stopped_p"]).sum()) >= 8, kw
        assert int((p & (r["off_s"] > r["off_e"])).sum()) >= 8 and int((p & (r["off_e"] > r["off_s"])).sum()) >= 8, kw
        hz, vt = p & r["horizontal"], p & ~r["horizontal"]
        x_lo, x_hi = np.maximum(xs - r["dist_m"], 0), np.minimum(xs + r["dist_p"], W - 1)
        assert (hz & ((x_lo // 128 != xs // 128) | (x_hi // 128 != xs // 128))).any(), "no walk crosses a tile border in x"
        y_lo, y_hi = np.maximum(ys - r["dist_m"], 0), np.minimum(ys + r["dist_p"], Hh - 1)
        assert (vt & (((Hh - 1 - y_lo) // 16 != tile_row) | ((Hh - 1 - y_hi) // 16 != tile_row))).any(), "no walk crosses a tile border in y"
    for kw in AC.edge_params():                           # the ends of the ranges
        r = AC.rule_np(fb, **kw)
        assert np.array_equal(T.aa_host(fb, T.aa_params(**kw)), r["out"])
    assert np.array_equal(AC.rule_np(fb, contrast_min=0, contrast_rel=0)["passed"], _not_flat(fb)), "thresholds of 0 pass all but flat pixels"


def _not_flat(fb):
    lum = AC.luma_np(fb)
    pad = np.pad(lum, 1, mode="edge")
    five = np.stack([pad[1:-1, 1:-1], pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]])
    return five.max(0) != five.min(0)


def test_the_flags_case_is_not_vacuous(built, small_synthetic):
    """512 x 64 with AC.FLAGS_AT: some tile without a drawn pixel takes colour from a neighbour's edge, others take none."""
    import tiny_renderer_amd as T
    from tests import outline_cases as OC
    from tests.test_composite import tiles_any
    fb, z = oracle_frame(small_synthetic, 512, 64, T.apply_instances(small_synthetic[0], AC.FLAGS_AT))
    empty = ~tiles_any(OC.bits(z) != OC.F32_MIN_BITS)
    assert not fb[::-1][np.repeat(np.repeat(empty, 16, 0), 128, 1)].any(), "an empty tile is black"
    lit = tiles_any(T.aa_host(fb, T.aa_params()).any(-1)[::-1])
    assert (empty & lit).any() and (empty & ~lit).any()
