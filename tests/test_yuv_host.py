"""The YUV rule on the host: tr_yuv_host, the tables, tr_yuv_bytes / tr_yuv_plane, the refusals and Y4MWriter.

tests/yuv_cases.py restates the rule in numpy int64 from the header's text and derives the four tables in exact fractions;
everything here needs no GPU.  tests/test_yuv.py compares the device with tr_yuv_host."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import yuv_cases as YC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISSUE_TABLES = {
    ("bt601", "full"): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329), 0),
    ("bt601", "limited"): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681), 16),
    ("bt709", "full"): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005), 0),
    ("bt709", "limited"): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639), 16),
}


@pytest.fixture(scope="module")
def T(built):
    import tiny_renderer_amd as T
    return T


def flat(planes):
    return np.concatenate([p.reshape(-1) for p in planes])


@pytest.mark.parametrize("matrix,rng", YC.TABLES)
def test_the_librarys_tables_are_the_derived_ones_and_their_rows_sum(T, matrix, rng):
    y, u, v, y0 = YC.derive(matrix, rng)
    assert T.yuv_coefficients(matrix, rng) == (y, u, v, y0) == ISSUE_TABLES[(matrix, rng)]
    assert sum(y) == (65536 if rng == "full" else YC.nearest(YC.Fraction(219, 255) * 65536)) and sum(u) == 0 and sum(v) == 0
    text = open(os.path.join(REPO, "include", "tiny_renderer.h")).read()
    for row in (y, u, v):
        assert re.search(r"\s+".join(str(c) for c in row), text), "the header's table does not hold %r" % (row,)


@pytest.mark.parametrize("layout", YC.LAYOUTS)
@pytest.mark.parametrize("matrix,rng", YC.TABLES)
def test_host_rule_equals_the_numpy_rule_in_every_byte(T, layout, matrix, rng):
    for W, Hh in YC.HOST_SIZES:
        rgb = YC.noise(W, Hh)
        keep = rgb.copy()
        got = T.yuv_host(rgb, layout, matrix, rng)
        want = YC.rule_np(rgb, layout, matrix, rng)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), "%dx%d: %d bytes differ" % (W, Hh, int((g != w).sum()))
        assert np.array_equal(rgb, keep)
        whole = T.yuv_host(rgb, layout, matrix, rng, flat=True)
        assert whole.size == YC.nbytes(W, Hh, layout) == T.yuv_bytes(W, Hh, layout) and np.array_equal(whole, flat(want))


@pytest.mark.parametrize("matrix,rng", YC.TABLES)
def test_greys_black_white_primaries_and_the_clamp(T, matrix, rng):
    greys = np.repeat(np.arange(256, dtype=np.uint8), 3).reshape(16, 16, 3)
    for layout in YC.LAYOUTS:
        planes = T.yuv_host(greys, layout, matrix, rng)
        if rng == "full":
            assert np.array_equal(planes[0], greys[..., 0]), "a grey v gives Y = v in full range"
        else:
            assert planes[0].min() == 16 and planes[0].max() == 235
        assert all((p == 128).all() for p in planes[1:]), "a grey gives U = V = 128"
    y0 = 0 if rng == "full" else 16
    black, white = np.zeros((2, 2, 3), np.uint8), np.full((2, 2, 3), 255, np.uint8)
    for layout in ("i420", "i444"):
        y, u, v = T.yuv_host(black, layout, matrix, rng)
        assert (y == y0).all() and (u == 128).all() and (v == 128).all(), "black gives (y0, 128, 128)"
        y, u, v = T.yuv_host(white, layout, matrix, rng)
        assert (y == (255 if rng == "full" else 235)).all() and (u == 128).all() and (v == 128).all()
    # pure primaries: a 2 x 2 block (4:2:0 and 4:4:4) and a 1-pixel-wide odd edge of blue (3 x 2: the last column twice)
    top = 256 if rng == "full" else 240
    blue, red = np.zeros((2, 2, 3), np.uint8), np.zeros((2, 2, 3), np.uint8)
    blue[..., 2], red[..., 0] = 255, 255
    for layout in ("i420", "i444"):
        raw_b, raw_r = YC.rule_np(blue, layout, matrix, rng, raw=True), YC.rule_np(red, layout, matrix, rng, raw=True)
        assert (raw_b[1] == top).all() and (raw_r[2] == top).all(), "pure blue's U and pure red's V before the clamp"
        assert (T.yuv_host(blue, layout, matrix, rng)[1] == min(top, 255)).all() and (T.yuv_host(red, layout, matrix, rng)[2] == min(top, 255)).all()
    edge = np.zeros((2, 3, 3), np.uint8)
    edge[:, 2, 2] = 255
    raw = YC.rule_np(edge, "i420", matrix, rng, raw=True)
    assert raw[1][0, 1] == top and raw[1][0, 0] == 128, "the odd edge's blue column counts twice"
    assert T.yuv_host(edge, "i420", matrix, rng)[1][0, 1] == min(top, 255)
    # nothing goes negative and limited range stays within its bounds, over the cube's corners and edges' middles
    lattice = np.array([[r, g, b] for r in (0, 128, 255) for g in (0, 128, 255) for b in (0, 128, 255)], np.uint8).reshape(1, 27, 3)
    for layout in ("i420", "i444"):
        rawp = YC.rule_np(np.repeat(lattice, 2, 0), layout, matrix, rng, raw=True)
        assert all(p.min() >= 0 for p in rawp) and all(p.max() <= 256 for p in rawp)
        if rng == "limited":
            assert rawp[0].min() >= 16 and rawp[0].max() <= 235 and all(16 <= p.min() and p.max() <= 240 for p in rawp[1:])
    # every accumulator stays below 2^27
    y, u, v, _ = YC.derive(matrix, rng)
    assert max(sum(abs(c) for c in row) for row in (u, v)) * 1020 + (128 << 18) + (1 << 17) < 1 << 27
    assert sum(y) * 255 + (16 << 16) + 32768 < 1 << 27


@pytest.mark.parametrize("matrix,rng", YC.TABLES)
def test_y_is_within_one_of_the_real_matrix_over_a_colour_lattice(T, matrix, rng):
    """|Y - round(float64 matrix)| <= 1 over 52^3 colours: rounding the coefficients moves the sum by less than 3 * 255 *
    0.5 / 65536 < 0.006 (1.5 units of green's adjustment included: < 0.01), so the two roundings differ by at most 1."""
    v = np.linspace(0, 255, 52).round().astype(np.uint8)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    rgb = np.stack([r, g, b], -1).reshape(52, 52 * 52, 3)
    yr, ur, vr, y0 = YC.real_matrix(matrix, rng)
    got = T.yuv_host(rgb, "i444", matrix, rng)
    f = rgb.astype(np.float64)
    for plane, row, off in ((got[0], yr, y0), (got[1], ur, 128.0), (got[2], vr, 128.0)):
        want = np.clip(np.floor(f @ row + off + 0.5), 0, 255)
        assert np.abs(plane.astype(np.float64) - want).max() <= 1


def test_layouts_agree_with_each_other(T):
    rgb = YC.noise(131, 19)
    for matrix, rng in YC.TABLES:
        i420, nv12, i444 = (T.yuv_host(rgb, lay, matrix, rng) for lay in YC.LAYOUTS)
        assert np.array_equal(nv12[1][..., 0], i420[1]) and np.array_equal(nv12[1][..., 1], i420[2]), "NV12's pairs are I420's planes interleaved"
        assert np.array_equal(nv12[0], i420[0]) and np.array_equal(i444[0], i420[0]), "Y is the same in every layout"


def test_bytes_and_planes_agree_with_the_table(T):
    L = T.load_library()
    for W, Hh in YC.HOST_SIZES + ((8192, 8192), (8191, 3)):
        cw, ch = (W + 1) // 2, (Hh + 1) // 2
        want = {"i420": [(0, W, Hh, 1), (W * Hh, cw, ch, 1), (W * Hh + cw * ch, cw, ch, 1)],
                "nv12": [(0, W, Hh, 1), (W * Hh, cw, ch, 2)],
                "i444": [(0, W, Hh, 1), (W * Hh, W, Hh, 1), (2 * W * Hh, W, Hh, 1)]}
        for k, layout in enumerate(YC.LAYOUTS):
            assert T.yuv_bytes(W, Hh, layout) == YC.nbytes(W, Hh, layout) == sum(w * h * st for _, w, h, st in want[layout])
            for plane, row in enumerate(want[layout]):
                off, pw, ph, step = C.c_size_t(), C.c_uint32(), C.c_uint32(), C.c_uint32()
                assert L.tr_yuv_plane(W, Hh, k, plane, C.addressof(off), C.addressof(pw), C.addressof(ph), C.addressof(step)) == 0
                assert (off.value, pw.value, ph.value, step.value) == row
    flat_ = np.arange(T.yuv_bytes(7, 5, "nv12"), dtype=np.uint8)
    y, uv = T.yuv_planes(flat_, 7, 5, "nv12")
    assert y.shape == (5, 7) and uv.shape == (3, 4, 2) and y.base is not None and uv[0, 0, 0] == 35
    assert np.shares_memory(y, flat_) and np.shares_memory(uv, flat_), "the planes are views"


def test_every_refusal_carries_its_text(T):
    from tiny_renderer_amd import _lib
    L = T.load_library()
    text = lambda: L.tr_last_error().decode()
    rgb, out = np.zeros((4, 4, 3), np.uint8), np.zeros(64, np.uint8)
    good = T.yuv_params()
    q = C.addressof(good)
    assert L.tr_yuv_host(4, 4, rgb.ctypes.data, q, out.ctypes.data) == 0
    for fields, why in (((3, 0, 0, 0), ": layout must be TR_YUV_I420, TR_YUV_NV12 or TR_YUV_I444"), ((0, 2, 0, 0), ": matrix must be TR_YUV_BT601 or TR_YUV_BT709"),
                        ((0, 0, 2, 0), ": range must be TR_YUV_FULL or TR_YUV_LIMITED"), ((0, 0, 0, 1), ": flags must be 0")):
        bad = T.YuvParams(*fields)
        assert L.tr_yuv_host(4, 4, rgb.ctypes.data, C.addressof(bad), out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_yuv_host" + why
    assert L.tr_yuv_host(4, 4, rgb.ctypes.data, None, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_yuv_host: null argument"
    assert L.tr_yuv_host(4, 4, None, q, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_yuv_host: null argument"
    assert L.tr_yuv_host(4, 4, rgb.ctypes.data, q, None) == _lib.TR_E_INVALID and text() == "tr_yuv_host: null argument"
    assert L.tr_yuv_host(4, 4, rgb.ctypes.data, q, rgb.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_yuv_host: out is rgb (the sizes differ: not in place)"
    for w, h in ((0, 4), (4, 0), (8193, 4), (4, 8193)):
        assert L.tr_yuv_host(w, h, rgb.ctypes.data, q, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_yuv_host: width and height must be 1..8192"
        assert L.tr_yuv_bytes(w, h, 0) == 0 and text() == "tr_yuv_bytes: an unknown layout, or width and height not 1..8192"
    assert L.tr_yuv_bytes(4, 4, 3) == 0
    off, pw, ph, step = C.c_size_t(), C.c_uint32(), C.c_uint32(), C.c_uint32()
    ptrs = [C.addressof(v) for v in (off, pw, ph, step)]
    assert L.tr_yuv_plane(4, 4, 1, 2, *ptrs) == _lib.TR_E_INVALID and text() == "tr_yuv_plane: the layout has no such plane"
    assert L.tr_yuv_plane(4, 4, 0, 3, *ptrs) == _lib.TR_E_INVALID
    assert L.tr_yuv_plane(4, 4, 5, 0, *ptrs) == _lib.TR_E_INVALID and text() == "tr_yuv_plane: layout must be TR_YUV_I420, TR_YUV_NV12 or TR_YUV_I444"
    assert L.tr_yuv_plane(4, 4, 0, 0, None, *ptrs[1:]) == _lib.TR_E_INVALID and text() == "tr_yuv_plane: null argument"
    assert L.tr_yuv_coefficients(2, 0, out.ctypes.data) == _lib.TR_E_INVALID and L.tr_yuv_coefficients(0, 0, None) == _lib.TR_E_INVALID
    for kw in (dict(layout="i422"), dict(matrix="bt2020"), dict(range="tv"), dict(layout=True)):
        with pytest.raises(ValueError):
            T.yuv_params(**kw)
    with pytest.raises(ValueError):
        T.yuv_host(np.zeros((4, 4), np.uint8))
    # null scenes, without a GPU
    assert L.tr_scene_to_yuv(None, q, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_to_yuv: null scene"
    assert L.tr_scene_to_yuv_from(None, rgb.ctypes.data, 4, 4, q, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_to_yuv_from: null scene"
    assert L.tr_scene_get_yuv(None, q, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_yuv: null scene"


@pytest.mark.parametrize("layout,rng,tag", [("i420", "limited", "C420jpeg"), ("i444", "full", "C444")])
def test_y4m_writer_round_trip(T, tmp_path, layout, rng, tag):
    W, Hh = 7, 5
    path = str(tmp_path / "x.y4m")
    frames = [YC.noise(W, Hh, k) for k in range(3)]
    with T.Y4MWriter(path, W, Hh, 25, layout, rng) as w:
        w.write(T.yuv_host(frames[0], layout, "bt709", rng))                # the tuple of planes
        w.write(T.yuv_host(frames[1], layout, "bt709", rng, flat=True))     # the flat array
        w.write(T.yuv_host(frames[2], layout, "bt709", rng, flat=True))
        with pytest.raises(ValueError):
            w.write(np.zeros(3, np.uint8))
        assert w.frames == 3
    fields, got = YC.parse_y4m(path)
    assert fields == ["YUV4MPEG2", "W7", "H5", "F25:1", "Ip", "A1:1", tag, "XCOLORRANGE=" + rng.upper()]
    assert len(got) == 3 and os.path.getsize(path) == len(" ".join(fields)) + 1 + 3 * (6 + YC.nbytes(W, Hh, layout))
    for f, g in zip(frames, got):
        assert np.array_equal(g, YC.flat_np(f, layout, "bt709", rng))
    with T.Y4MWriter(path, W, Hh, (30000, 1001)) as w:
        pass
    assert YC.parse_y4m(path)[0][3] == "F30000:1001"
    with pytest.raises(ValueError, match="NV12"):
        T.Y4MWriter(path, W, Hh, 30, "nv12")
    for bad in (0, -1, 2.5, (30, 0)):
        with pytest.raises(ValueError):
            T.Y4MWriter(path, W, Hh, bad)


@pytest.mark.skipif(shutil.which(os.environ.get("CXX", "g++")) is None, reason="no host C++ compiler")
def test_the_host_check_program_compiles_and_passes(tmp_path):
    """scripts/yuv_host_check.cpp, built for the host without a sanitizer (the same program is what runs under
    -fsanitize=address,undefined by hand: its header has the line)."""
    exe = str(tmp_path / "yuv_host_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(REPO, "include"),
                           "-I" + os.path.join(REPO, "tiny_renderer_amd", "csrc"), os.path.join(REPO, "scripts", "yuv_host_check.cpp"), "-o", exe])
    done = subprocess.run([exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    m = re.search(r"yuv: (\d+) images, (\d+) bytes, 0 mismatches", done.stdout)
    assert m and int(m.group(1)) == 480
