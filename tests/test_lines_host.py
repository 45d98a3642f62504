"""The rule of lines on the host: tr_lines_host against tests/lines_cases.py's numpy restatement of the header's text, the
rule's facts, tr_project_points against the oracle's z buffer, the refusals with their full texts, the builders, and the
conditions of the GPU cases asserted on the oracle's frames of those very cases.

Everything here needs no GPU.  tests/test_lines.py compares the device with tr_lines_host."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import lines_cases as LN
from tests import view_cases as VC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, Hh = 37, 23            # the frame of the small cases


@pytest.fixture(scope="module")
def T(built):
    import tiny_renderer_amd as T
    return T


def frame_and_depth(seed=1, w=W, h=Hh):
    """A random frame and a depth: a disc drawn with depths in 0..100, f32::MIN around it, and a NaN in its first row."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (xx - w // 2) ** 2 + (yy - h // 2) ** 2 < (min(w, h) // 2) ** 2
    z = np.where(disc, rng.random((h, w), np.float32) * np.float32(100.0), LN.F32_MIN).astype(np.float32)
    row = np.flatnonzero(disc.any(1))[0]
    z[row, np.flatnonzero(disc[row])[0]] = np.float32(np.nan)
    return rgb, z


def params(T, combo):
    w, test, painter, opacity, bias = combo
    return T.lines_params(w, opacity, test, painter, bias)


def one(T, x0, y0, z0, x1, y1, z1, colour=(255, 255, 255, 255)):
    return T.lines_table([[x0, y0]], [z0], [[x1, y1]], [z1], colour)


def oracle_frame(T, small_synthetic, w, h):
    from oracle import oracle as O
    mesh = T.apply_instances(small_synthetic[0], LN.table(w, h))
    s = O.Scene(w, h, mesh, small_synthetic[1], "phong")
    s.clear()
    s.set_light_direction(H.light(LN.LIGHT)), s.set_camera(*H.camera(LN.CAM)), s.render()
    z, fb = s.z_f32(), s.get_frame_buffer()
    s.close()
    return fb, z


def test_entry_points_declared_exported_and_typed(T):
    from tiny_renderer_amd import _lib
    header = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    for word in ("} tr_line;", "} tr_lines_params;", "#define TR_LINES_MAX_N (1u << 20)", "#define TR_LINES_DEPTH_TEST 0x1u", "#define TR_LINES_PAINTER 0x2u",
                 "#define TR_ABI_VERSION 3", "int tr_scene_set_lines(tr_scene *s, uint32_t n, const tr_line *lines);",
                 "int tr_scene_lines(tr_scene *s, const tr_lines_params *p, void *out /* or NULL */);",
                 "int tr_scene_get_lined(tr_scene *s, const tr_lines_params *p, uint8_t *rgb);",
                 "int tr_scene_debug_line_bins(tr_scene *s, uint32_t *n_tiles, uint64_t *n_entries);",
                 "int tr_project_points(const tr_uniforms *u, uint32_t n, const float *xyz, int32_t *xy, float *z, uint8_t *ok);"):
        assert word in header, word
    raw = C.CDLL(_lib.library_path())
    exports = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "exports.map")).read()
    assert "global: tr_*;" in exports, "the map exports the tr_ names"
    sigs = {"tr_scene_set_lines": [C.c_void_p, C.c_uint32, C.c_void_p], "tr_scene_lines": [C.c_void_p] * 3, "tr_scene_get_lined": [C.c_void_p] * 3,
            "tr_lines_host": [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p],
            "tr_scene_debug_line_bins": [C.c_void_p] * 3, "tr_project_points": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]}
    for name, args in sigs.items():
        assert hasattr(raw, name), name + " is not exported"
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
    assert C.sizeof(T.LinesParams) == 32 and T.LINE_DTYPE.itemsize == 32
    assert T.load_library().tr_abi_version() == 3
    src = open(os.path.join(REPO, "tiny_renderer_amd", "csrc", "tr_scene.cpp")).read()
    assert "sizeof(tr_lines_params) == 32" in src and src.count('"k_lines" };') == 1, "K_LINES ends the profile's kernel list"
    for name in ("lines_host", "lines_params", "lines_table", "project_points", "mesh_edges", "wireframe_lines", "lines_box", "lines_axes", "lines_grid",
                 "lines_polyline"):
        assert hasattr(T, name) and name in T.__all__, name
    for name in ("set_lines", "lines", "get_lined", "project", "debug_line_bins"):
        assert callable(getattr(T.Scene, name)), name


@pytest.mark.parametrize("w,h", LN.GPU_SIZES, ids=["%dx%d" % s for s in LN.GPU_SIZES])
def test_host_rule_equals_the_numpy_rule_on_the_oracles_frames(T, small_synthetic, w, h):
    """The oracle's frame of each GPU case with that case's 300 segments: tr_lines_host equals the restatement in every
    byte under every combination the GPU cases run, and the cases reach what they are for -- at width 1 under the test
    at least 5 % of the pixels with a candidate have one that the test rejects and at least 5 % one that it passes, at
    least 1 % of ALL pixels have two or more survivors, and keys tie (two survivors of a pixel share the winner's key)."""
    fb, z = oracle_frame(T, small_synthetic, w, h)
    lines = LN.segments(w, h)
    keep = (fb.copy(), z.copy(), lines.copy())
    kinds = np.abs(np.stack([lines[k].astype(np.int64) for k in ("x0", "y0", "x1", "y1")]))
    assert (kinds == LN.LIMIT).any() and ((lines["x0"] == lines["x1"]) & (lines["y0"] == lines["y1"])).any()
    census = {}
    LN.rule_np(fb, z, lines, 1, True, False, 256, 0.0, census)
    touched = (census["survivors"] + census["rejected"]) > 0
    n_touched = int(touched.sum())
    assert 20 * int((census["rejected"] > 0).sum()) >= n_touched, "%d of %d touched pixels reject a candidate" % (int((census["rejected"] > 0).sum()), n_touched)
    assert 20 * int((census["survivors"] > 0).sum()) >= n_touched
    assert 100 * int((census["survivors"] >= 2).sum()) >= w * h, "%d of %d pixels have two survivors" % (int((census["survivors"] >= 2).sum()), w * h)
    assert (census["tied"] >= 2).any(), "no two survivors of a pixel tie in key"
    for combo in LN.COMBOS:
        want = LN.rule_np(fb, z, lines, *combo[:3], combo[3], combo[4])
        assert not np.array_equal(want, fb)
        got = T.lines_host(fb, z, lines, params(T, combo))
        assert np.array_equal(got, want), "%r: %d bytes differ" % (combo, int((got != want).sum()))
        assert np.array_equal(T.lines_host(fb, z, lines, params(T, combo), in_place=True), want), "out == rgb, %r" % (combo,)
        if not combo[1]:
            assert np.array_equal(T.lines_host(fb, None, lines, params(T, combo)), want), "no depth is read without the test"
    assert np.array_equal(fb, keep[0]) and np.array_equal(LN.bits(z), LN.bits(keep[1])) and np.array_equal(lines, keep[2])


def test_a_segment_and_its_reverse_give_equal_images(T):
    rgb, z = frame_and_depth()
    lines = LN.segments(W, Hh, 120, seed=5)
    for combo in LN.COMBOS:
        a, b = T.lines_host(rgb, z, lines, params(T, combo)), T.lines_host(rgb, z, LN.reverse(lines), params(T, combo))
        assert np.array_equal(a, b), combo
        assert np.array_equal(a, LN.rule_np(rgb, z, lines, *combo[:3], combo[3], combo[4]))


def test_endpoints_are_covered_and_a_width_covers_w_pixels_a_step(T):
    big = 101
    black = np.zeros((big, big, 3), np.uint8)
    rng = np.random.default_rng(9)
    for _ in range(60):
        x0, y0, x1, y1 = (int(v) for v in rng.integers(20, 80, 4))
        seg = one(T, x0, y0, 1.0, x1, y1, 2.0)
        out = T.lines_host(black, None, seg, T.lines_params(1, depth_test=False))
        drawn = out[::-1].any(-1)          # [y, x], y up
        assert drawn[y0, x0] and drawn[y1, x1], "an endpoint is not covered"
        n = max(abs(x1 - x0), abs(y1 - y0))
        assert int(drawn.sum()) == n + 1, "one pixel a step"
        xmajor = abs(x1 - x0) >= abs(y1 - y0)
        for w in range(1, 16):
            d = T.lines_host(black, None, seg, T.lines_params(w, depth_test=False))[::-1].any(-1)
            per_step = d.sum(0 if xmajor else 1)
            assert set(per_step[per_step > 0]) == {w} and int((per_step > 0).sum()) == n + 1, "width %d covers %r pixels a step" % (w, set(per_step))
            if n == 0:
                lo, hi = x0 - (w - 1) // 2, x0 + w // 2       # (n == 0 is x major: the offsets run along y)
                assert d[y0 - (w - 1) // 2:y0 + w // 2 + 1, x0].all() and lo <= x0 <= hi


def test_opacity_0_and_alpha_0_leave_the_frame(T):
    rgb, z = frame_and_depth(2)
    lines = LN.segments(W, Hh, 100, seed=3)
    for test in (False, True):
        assert np.array_equal(T.lines_host(rgb, z, lines, T.lines_params(3, 0, test)), rgb)
        clear = lines.copy()
        clear["rgba"][:, 3] = 0
        assert np.array_equal(T.lines_host(rgb, z, clear, T.lines_params(3, 256, test)), rgb)
        opaque = lines.copy()
        opaque["rgba"][:, 3] = 255
        out = T.lines_host(rgb, z, opaque, T.lines_params(1, 256, test))
        won = LN.winners(z, opaque, 1, test)[::-1]
        assert np.array_equal(out[won != 0], opaque["rgba"][(won[won != 0] & np.uint64(0xFFFFFFFF)).astype(np.int64) - 1][:, :3]), "alpha 255 at opacity 256 is the colour"
    assert np.array_equal(T.lines_host(rgb, z, lines[:0], T.lines_params()), rgb), "n == 0"


def test_painter_equals_drawing_one_call_at_a_time(T):
    rgb, z = frame_and_depth(4)
    lines = LN.segments(W, Hh, 60, seed=8)
    lines["rgba"][:, 3] = 255            # (opaque: drawing over is replacing, as a winner replaces)
    for w in (1, 4):
        want = rgb.copy()
        for i in range(lines.shape[0]):
            want = T.lines_host(want, None, lines[i:i + 1], T.lines_params(w, depth_test=False))
        assert np.array_equal(T.lines_host(rgb, z, lines, T.lines_params(w, depth_test=False, painter=True)), want)
    # under the test PAINTER still orders the survivors by index
    got = T.lines_host(rgb, z, lines, T.lines_params(2, painter=True))
    assert np.array_equal(got, LN.rule_np(rgb, z, lines, 2, True, True))


def test_nan_and_f32_min_depths_pass_and_bias_moves_a_coincident_line(T):
    rgb = np.zeros((3, 8, 3), np.uint8)
    z = np.full((3, 8), 50.0, np.float32)
    z[1, 2], z[1, 3] = np.float32(np.nan), LN.F32_MIN
    seg = one(T, 0, 1, 10.0, 7, 1, 10.0)
    out = T.lines_host(rgb, z, seg, T.lines_params())[::-1].any(-1)
    assert out[1].tolist() == [False, False, True, True, False, False, False, False], "only the NaN and the f32::MIN depth pass"
    # a line ON the surface is hidden (zl <= zbuf) until the bias lifts it
    on = one(T, 0, 1, 50.0, 7, 1, 50.0)
    z[:] = 50.0
    assert not T.lines_host(rgb, z, on, T.lines_params()).any()
    assert not T.lines_host(rgb, z, on, T.lines_params(depth_bias=-0.5)).any()
    assert T.lines_host(rgb, z, on, T.lines_params(depth_bias=0.5))[::-1].any(-1)[1].all()
    # ties go to the greatest index; the nearer (larger) depth wins whatever the index
    two = np.concatenate([one(T, 0, 1, 60.0, 7, 1, 60.0, (9, 0, 0, 255)), one(T, 0, 1, 60.0, 7, 1, 60.0, (0, 9, 0, 255)), one(T, 3, 0, 55.0, 3, 2, 55.0, (0, 0, 9, 255))])
    out = T.lines_host(rgb, z, two, T.lines_params())[::-1]
    assert (out[1] == (0, 9, 0)).all() and tuple(out[0, 3]) == (0, 0, 9)
    assert tuple(T.lines_host(rgb, z, two, T.lines_params(painter=True))[::-1][1, 3]) == (0, 0, 9)


def test_coordinates_at_the_limit_and_the_exact_floor(T):
    """Segments from corner to corner of the coordinate range: 2 k db + n reaches 2^43, and the rule's floor division is
    exact there (the restatement divides Python-sized integers)."""
    rgb, z = frame_and_depth(6, 64, 40)
    L = LN.LIMIT
    ends = [(-L, -L, L, L), (-L, L, L, -L), (-L, -L + 13, L, L - 7), (-L + 3, L, L, -L + 1), (5, -L, 40, L), (-L, 20, L, 21), (-L, 0, L, 39), (0, -L, 63, L)]
    lines = np.concatenate([one(T, a, b, 0.0, c, d, 100.0, (200, 100, 50, 255)) for a, b, c, d in ends])
    for w in (1, 15):
        got = T.lines_host(rgb, z, lines, T.lines_params(w, depth_test=False))
        assert np.array_equal(got, LN.rule_np(rgb, None, lines, w, False)) and not np.array_equal(got, rgb)
        got = T.lines_host(rgb, z, lines, T.lines_params(w))
        assert np.array_equal(got, LN.rule_np(rgb, z, lines, w, True))


@pytest.mark.parametrize("case", VC.DEFINED_CAMERAS)
def test_projected_vertices_have_the_oracles_depth_bit_for_bit(T, case):
    """One-triangle meshes under view_cases' cameras: the oracle draws the triangle, and at each vertex's own pixel its z
    buffer holds the vertex's depth (the barycentric weights there are 1, 0, 0) -- the very bits tr_project_points gives."""
    from oracle import oracle as O
    cams = [VC.CAMERAS[case]]
    checked = 0
    w, h = 96, 64
    rng = np.random.default_rng(12)
    tex = [np.full((4, 4, 3), 200, np.uint8)] * 4
    for cam in cams:
        view = cam
        for _ in range(6):
            pos = ((rng.random((3, 3), np.float32) - np.float32(0.5)) * np.float32(1.6)).astype(np.float32)
            pos[:, 2] *= np.float32(0.2)
            mesh = {"pos": pos, "tex": np.zeros((1, 3), np.float32), "nrm": np.array([[0, 0, 1]], np.float32),
                    "idx": np.array([[0, 0, 0, 1, 0, 0, 2, 0, 0]], np.uint32)}
            st, u = T.prepare_uniforms(0, w, h, H.light(LN.LIGHT), *view)
            assert st == 0
            xy, zp, ok = T.project_points(u, pos)
            for order in ((0, 1, 2), (0, 2, 1)):       # (one winding faces the camera)
                m = dict(mesh, idx=mesh["idx"].reshape(3, 3)[list(order)].reshape(1, 9))
                s = O.Scene(w, h, m, tex, "phong")
                s.clear()
                s.set_light_direction(H.light(LN.LIGHT)), s.set_camera(*view), s.render()
                z = s.z_f32()
                s.close()
                if not (LN.bits(z) != LN.F32_MIN_BITS).any():
                    continue
                for k in range(3):
                    x, y = int(xy[k, 0]), int(xy[k, 1])
                    if ok[k] and 0 <= x < w and 0 <= y < h and LN.bits(z)[y, x] != LN.F32_MIN_BITS:
                        assert LN.bits(z)[y, x] == LN.bits(zp[k:k + 1])[0], "vertex %d: z %r, projected %r" % (k, z[y, x], zp[k])
                        checked += 1
    # (the cameras that look away from the origin put these small triangles outside the frame: nothing to compare there)
    assert checked >= 3 or case in ("behind7", "straddle", "straddle_moved"), "no vertex's pixel was drawn: the case shows nothing"


def test_project_points_refuses_what_a_line_cannot_hold(T):
    st, u = T.prepare_uniforms(0, 96, 64, H.light(LN.LIGHT), *H.camera(LN.CAM))
    assert st == 0
    wide = type(u)()
    for k, v in enumerate((1.0e7, 1.0, 1.0, 1.0)):
        wide.vpmv[5 * k] = v               # x' = 1e7 x: past 2^20 from x = 0.2 on
    xy, z, ok = T.project_points(wide, np.array([[0.1, 3, 5], [0.2, 3, 5], [-0.2, 3, 5], [0, 2.0 ** 21, 5], [0, 3, 2.0 ** 101], [np.nan, 0, 0]], np.float32))
    assert ok.tolist() == [True, False, False, False, False, False] and not xy[1:].any() and not z[1:].any()
    assert xy[0].tolist() == [1000000, 3] and z[0] == 5.0
    assert T.project_points(u, np.zeros((1, 3), np.float32))[2].all()
    zero = type(u)()
    assert not T.project_points(zero, np.zeros((2, 3), np.float32))[2].any(), "w == 0"
    with pytest.raises(ValueError):
        T.project_points(u, np.zeros((2, 2), np.float32))


def test_every_refusal_text(T):
    from tiny_renderer_amd import _lib
    L = T.load_library()
    rgb, z = frame_and_depth()
    out = np.empty_like(rgb)
    good = one(T, 0, 0, 1.0, 5, 5, 2.0)

    def call(p, n=1, lines=good, w=W, h=Hh, src=rgb, zz=z):
        return L.tr_lines_host(w, h, src.ctypes.data if src is not None else None, zz.ctypes.data if zz is not None else None,
                               C.addressof(p) if p is not None else None, n, lines.ctypes.data if lines is not None else None, out.ctypes.data)

    def text():
        return L.tr_last_error().decode()

    ok = T.lines_params()
    assert call(ok) == 0
    for fields, why in (((0, 256, 1, 0.0), "width must be 1..15"), ((16, 256, 1, 0.0), "width must be 1..15"), ((1, 257, 1, 0.0), "opacity must be 0..256"),
                        ((1, 256, 4, 0.0), "unknown flags"), ((1, 256, 1, float("inf")), "depth_bias must be finite"), ((1, 256, 1, float("nan")), "depth_bias must be finite")):
        bad = T.LinesParams(*fields, (C.c_uint32 * 4)())
        assert call(bad) == _lib.TR_E_INVALID and text() == "tr_lines_host: " + why
    for k in range(4):
        r = (C.c_uint32 * 4)()
        r[k] = 1
        assert call(T.LinesParams(1, 256, 1, 0.0, r)) == _lib.TR_E_INVALID and text() == "tr_lines_host: reserved must be 0"
    assert call(None) == _lib.TR_E_INVALID and text() == "tr_lines_host: null argument"
    assert call(ok, lines=None) == _lib.TR_E_INVALID and text() == "tr_lines_host: null table"
    assert call(ok, n=(1 << 20) + 1) == _lib.TR_E_INVALID and text() == "tr_lines_host: the table's length n must be 0..TR_LINES_MAX_N"
    assert call(ok, src=None) == _lib.TR_E_INVALID and text() == "tr_lines_host: null argument"
    assert call(ok, zz=None) == _lib.TR_E_INVALID and text() == "tr_lines_host: null argument"
    assert call(T.lines_params(depth_test=False), zz=None) == 0 and call(ok, n=0, lines=None) == 0
    for w, h in ((0, 4), (4, 0), (32769, 4)):
        assert call(ok, w=w, h=h) == _lib.TR_E_INVALID and text() == "tr_lines_host: the frame's width and height must be 1..32768"
    table = np.concatenate([good, good, good])
    for field, value, why in (("x0", (1 << 20) + 1, "coordinates must lie within +-2^20"), ("y1", -(1 << 20) - 1, "coordinates must lie within +-2^20"),
                              ("z0", np.float32(np.nan), "z must be finite with |z| <= 2^100"), ("z1", np.float32(np.inf), "z must be finite with |z| <= 2^100"),
                              ("z0", np.float32(2.0 ** 101), "z must be finite with |z| <= 2^100"), ("reserved", 7, "reserved must be 0")):
        bad = table.copy()
        bad[field][2] = value
        assert call(ok, 3, bad) == _lib.TR_E_INVALID and text() == "tr_lines_host: segment 2: " + why
    edge = table.copy()
    edge["x0"][1], edge["y0"][1], edge["z0"][1], edge["z1"][1] = 1 << 20, -(1 << 20), np.float32(2.0 ** 100), np.float32(-2.0 ** 100)
    assert call(ok, 3, edge) == 0, "the limits themselves are allowed"
    # the Python side says the same before the library is asked
    for kw, why in ((dict(width=0), "width must be 1..15"), (dict(width=True), "width must be 1..15"), (dict(opacity=257), "opacity must be 0..256"),
                    (dict(depth_bias=float("nan")), "depth_bias must be finite")):
        with pytest.raises(ValueError, match=re.escape("lines: " + why)):
            T.lines_params(**kw)
    for bad_call in (lambda: T.lines_host(rgb, z, good, T.ramp_params(0.0, 1.0)), lambda: T.lines_host(rgb, z[:3], good, ok),
                     lambda: T.lines_host(rgb, z, np.zeros((2, 8), np.int32), ok), lambda: T.lines_table([[0, 0]], [0.0], [[1, 1], [2, 2]], [0.0]),
                     lambda: T.lines_table([[0, 0]], [0.0], [[1, 1]], [0.0], (1, 2)), lambda: T.lines_polyline(np.zeros((1, 3))), lambda: T.lines_grid(0)):
        with pytest.raises(ValueError):
            bad_call()
    s = T.Scene.__new__(T.Scene)
    s.width, s.height, s._h, s._pinned = 64, 64, None, []
    with pytest.raises(ValueError):
        s.set_lines(np.zeros((2, 8), np.int32))
    with pytest.raises(ValueError):
        s.lines(params=T.ramp_params(0.0, 1.0))
    with pytest.raises(ValueError):
        s.project(np.zeros((1, 3), np.float32))


def test_the_builders(T, small_synthetic):
    mesh = small_synthetic[0]
    e = T.mesh_edges(mesh)
    p = np.asarray(mesh["idx"]).astype(np.int64)[:, (0, 3, 6)]
    want = {tuple(sorted((int(f[a]), int(f[b])))) for f in p for a, b in ((0, 1), (1, 2), (2, 0)) if f[a] != f[b]}
    assert e.shape == (len(want), 2) and {tuple(r) for r in e.tolist()} == want and (e[:, 0] < e[:, 1]).all()
    a, b = T.lines_box((-1, -2, -3), (1, 2, 3))
    assert a.shape == (12, 3) and b.shape == (12, 3) and ((a != b).sum(1) == 1).all(), "twelve axis-parallel edges"
    assert len({(tuple(x), tuple(y)) for x, y in zip(a.tolist(), b.tolist())}) == 12 and set(np.abs(a).reshape(-1, 3).max(0)) == {1.0, 2.0, 3.0}
    a, b = T.lines_axes(2.5)
    assert not a.any() and np.array_equal(b, np.eye(3, dtype=np.float32) * np.float32(2.5))
    a, b = T.lines_grid(2, 0.5, y=-1.0)
    assert a.shape == (10, 3) and (a[:, 1] == -1.0).all() and (b[:, 1] == -1.0).all() and np.abs(np.concatenate([a, b])[:, (0, 2)]).max() == 1.0
    assert ((a[:5, 0] == b[:5, 0]) & (a[:5, 2] == -b[:5, 2])).all() and ((a[5:, 2] == b[5:, 2]) & (a[5:, 0] == -b[5:, 0])).all()
    pts = np.arange(12, dtype=np.float32).reshape(4, 3)
    a, b = T.lines_polyline(pts)
    assert np.array_equal(a, pts[:-1]) and np.array_equal(b, pts[1:])
    a, b = T.lines_polyline(pts, closed=True)
    assert a.shape == (4, 3) and np.array_equal(b[-1], pts[0])
    t = T.lines_table([[1, 2], [3, 4]], [0.5, 1.5], [[5, 6], [7, 8]], [2.5, 3.5], (10, 20, 30))
    assert t.dtype == T.LINE_DTYPE and t["x1"].tolist() == [5, 7] and t["rgba"].tolist() == [[10, 20, 30, 255]] * 2 and not t["reserved"].any()

    class Cam:
        """What wireframe_lines asks of a scene."""
        width, height = 96, 64
        _camera, _light = H.camera(LN.CAM), H.light(LN.LIGHT)
        project = T.Scene.project

    cam = Cam()
    wf = T.wireframe_lines(cam, mesh, (1, 2, 3, 200))
    xy, zz, ok = cam.project(mesh["pos"])
    assert ok.all() and wf.shape[0] == e.shape[0] and np.array_equal(wf["x0"], xy[e[:, 0], 0]) and np.array_equal(wf["z1"], zz[e[:, 1]])
    assert (wf["rgba"] == (1, 2, 3, 200)).all()


@pytest.mark.skipif(shutil.which(os.environ.get("CXX", "g++")) is None, reason="no host C++ compiler")
def test_the_host_check_program_compiles_and_passes(tmp_path):
    """scripts/lines_host_check.cpp, built for the host without a sanitizer (the same program is what runs under
    -fsanitize=address,undefined by hand: its header has the line)."""
    exe = str(tmp_path / "lines_host_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           "-I" + os.path.join(REPO, "tiny_renderer_amd", "csrc"), os.path.join(REPO, "scripts", "lines_host_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    m = re.search(r"lines: (\d+) floor divisions, (\d+) frames, (\d+) binned tables, 0 mismatches", done.stdout)
    assert m and int(m.group(1)) >= 100000 and int(m.group(2)) >= 100 and int(m.group(3)) >= 50
