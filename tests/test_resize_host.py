"""The resize stage on the host, no GPU: the entry points are declared, exported and typed; tr_resize_taps -- the tables
k_resize is fed -- equals the rule restated in Python integers (tests/resize_cases.py) for every allowed pair of sizes up
to 40 and at sampled positions of large pairs; tr_resize_host equals numpy's int64 matrix products on random frames; the
anchors (the box filter at 2, 4 and 8, the copy, a white frame at the largest tap configuration, the listed weights) hold;
every refusal names its call and leaves `out` alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H
from tests import resize_cases as RC

LARGE_PAIRS = ((8192, 1024), (8192, 1025), (4096, 1920), (4095, 4096), (8192, 8191), (8191, 1024))


def test_entry_points_declared_exported_and_typed(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    header = open(os.path.join(H.REPO, "include", "tiny_renderer.h")).read()
    assert re.search(r"int\s+tr_scene_resize\(tr_scene \*s, const tr_resize_params \*p, void \*out\);", header)
    assert re.search(r"int\s+tr_scene_get_resized\(tr_scene \*s, const tr_resize_params \*p, uint8_t \*rgb\);", header)
    assert re.search(r"int\s+tr_resize_host\(uint32_t width, uint32_t height, const uint8_t \*rgb, const tr_resize_params \*p,\s*uint8_t \*out", header)
    assert re.search(r"int\s+tr_resize_taps\(uint32_t filter, uint32_t n_src, uint32_t n_dst, uint16_t \*first[^;]*uint16_t \*count[^;]*uint16_t \*weights[^;]*\);", header)
    assert re.search(r"typedef struct tr_resize_params \{\s*uint32_t width, height;[^}]*uint32_t filter;[^}]*uint32_t flags;[^}]*\} tr_resize_params;", header)
    for name, v in (("TR_RESIZE_AREA", "0u"), ("TR_RESIZE_BILINEAR", "1u"), ("TR_RESIZE_MAX_TAPS", "16")):
        assert re.search(r"#define %s %s\b" % (name, v), header), name
    assert "#define TR_ABI_VERSION 3" in header
    raw = C.CDLL(_lib.library_path())
    three, five = [C.c_void_p] * 3, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    for name, args in (("tr_scene_resize", three), ("tr_scene_get_resized", three), ("tr_resize_host", five),
                       ("tr_resize_taps", [C.c_uint32] * 3 + [C.c_void_p] * 3)):
        assert hasattr(raw, name), name + " is not exported"
        assert _lib.SYMBOLS[name] == (C.c_int, args), name
    assert C.sizeof(T.ResizeParams) == 16 and (T.scene.RESIZE_AREA, T.scene.RESIZE_BILINEAR, T.scene.RESIZE_MAX_TAPS) == (0, 1, 16)
    L = T.load_library()
    assert L.tr_abi_version() == 3
    p = T.ResizeParams(4, 4, 0, 0)
    assert L.tr_scene_resize(None, C.addressof(p), None) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_scene_resize: null scene"
    assert L.tr_scene_get_resized(None, C.addressof(p), None) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_scene_get_resized: null scene"
    for name in ("resize", "resize_into", "pinned_resized"):
        assert callable(getattr(T.Scene, name))


def check_pair(T, f, n, m, positions=()):
    """The library's tables of (n, m) against the rule: every entry against the int64 restatement, and at `positions`
    (all of them for a small m) against the rule in Python integers.  Returns the largest count."""
    first, count, weights = T.resize_taps(f, n, m)
    assert first.shape == (m,) and count.shape == (m,) and weights.shape == (m, RC.MAX_TAPS)
    f_np, c_np, w_np = RC.tables_np(f, n, m)
    assert np.array_equal(first, f_np) and np.array_equal(count, c_np) and np.array_equal(weights, w_np), (f, n, m)
    for X in range(m) if m <= 12 else positions:
        x0, w = RC.taps(f, n, m, X)
        assert (int(first[X]), int(count[X])) == (x0, len(w)), (f, n, m, X)
        assert weights[X, :len(w)].tolist() == w and not weights[X, len(w):].any(), (f, n, m, X)
        assert sum(w) == RC.ONE and min(w) >= 0 and 0 <= x0 and x0 + len(w) <= n, (f, n, m, X, w)
    # the sum, the sign (u16: nothing is negative) and the run inside [0, n), over the WHOLE table
    assert (weights.astype(np.int64).sum(1) == RC.ONE).all() and (count >= 1).all()
    assert (first.astype(np.int64) + count <= n).all()
    assert not (weights * (np.arange(RC.MAX_TAPS)[None, :] >= count[:, None])).any()
    return int(count.max())


SMALL_N, SMALL_M = 40, 8 * 40
# beyond SMALL_M every source size still meets the largest outputs, which is where a magnification is bounded
FAR_M = (321, 641, 1000, 4097, 8191, 8192)


def test_taps_equal_the_rule_in_python_integers(built):
    """Every allowed (N, M) with N <= 40 and M <= 320 -- every ratio from 1 / 8 to 8 of the largest N -- at every output
    index, and every N <= 40 against the far sizes FAR_M; then the large pairs.  (All M up to 8192 for every N <= 40 would
    be 4 * 10^10 taps: minutes even in numpy.  Beyond M = 8 N a run is 1 or 2 (area) or 2 or 3 (bilinear) taps long and
    only the position along the axis changes, which FAR_M and the large pairs sample.)  Every position is checked against
    the int64 restatement; the rule in Python integers is asked at every position of a small axis and at the ends, the
    middle and 12 drawn positions of a large one."""
    import tiny_renderer_amd as T
    rng = np.random.default_rng(7)
    most = {RC.AREA: 0, RC.BILINEAR: 0}
    pairs = 0

    def sample(m):
        return sorted(set([0, 1, 2, m // 2, m - 3, m - 2, m - 1] + rng.integers(0, m, 12).tolist()))

    for f in (RC.AREA, RC.BILINEAR):
        for n in range(1, SMALL_N + 1):
            for m in range(1, SMALL_M + 1):
                if RC.allowed(n, m):
                    most[f] = max(most[f], check_pair(T, f, n, m, sample(m) if (n + m) % 13 == 0 else ()))
                    pairs += 1
            for m in FAR_M:
                most[f] = max(most[f], check_pair(T, f, n, m, sample(m) if n % 8 == 0 else ()))
        for n, m in LARGE_PAIRS:
            most[f] = max(most[f], check_pair(T, f, n, m, sample(m)))
    print("largest tap count: area %d, bilinear %d (%d small pairs a filter)" % (most[RC.AREA], most[RC.BILINEAR], pairs // 2))
    assert pairs // 2 == sum(1 for n in range(1, SMALL_N + 1) for m in range(1, SMALL_M + 1) if RC.allowed(n, m)) > 12000
    assert max(most.values()) <= RC.MAX_TAPS == T.scene.RESIZE_MAX_TAPS
    assert most[RC.AREA] == 9 and most[RC.BILINEAR] == 16, "the cases hold the worst configuration"


def test_listed_weights(built):
    import tiny_renderer_amd as T
    first, count, w = T.resize_taps("bilinear", 5, 10)
    assert w[0, :1].tolist() == [4096] and count[0] == 1 and w[9, :1].tolist() == [4096] and count[9] == 1
    for X in range(1, 9):
        assert count[X] == 2 and first[X] == (X - 1) // 2
        assert w[X, :2].tolist() == ([3072, 1024] if X % 2 == 1 else [1024, 3072]), X
    first, count, w = T.resize_taps("area", 3, 1)
    assert (int(first[0]), int(count[0]), w[0, :3].tolist()) == (0, 3, [1365, 1366, 1365])
    for f in (2, 4, 8):
        first, count, w = T.resize_taps("area", 6 * f, 6)
        assert (count == f).all() and (first == np.arange(6) * f).all() and (w[:, :f] == 4096 // f).all()
    for filt in RC.FILTERS:
        first, count, w = T.resize_taps(filt, 37, 37)
        assert (count == 1).all() and (first == np.arange(37)).all() and (w[:, 0] == 4096).all(), "the same size is a copy"


SIZES = (((132, 17), (211, 9)), ((64, 48), (9, 300)), ((7, 5), (1, 1)), ((1, 1), (8, 8)), ((40, 33), (5, 66)), ((33, 40), (66, 5)))


@pytest.mark.parametrize("filt", RC.FILTERS)
@pytest.mark.parametrize("src,dst", SIZES, ids=["%dx%d-%dx%d" % (s + d) for s, d in SIZES])
def test_host_equals_numpy_on_random_frames(built, src, dst, filt):
    import tiny_renderer_amd as T
    rgb = np.random.default_rng(src[0] * 1000 + dst[0]).integers(0, 256, (src[1], src[0], 3), dtype=np.uint8)
    keep = rgb.copy()
    got = T.resize_host(rgb, dst[0], dst[1], filt)
    want = RC.resize_np(rgb, dst[0], dst[1], filt)
    assert got.shape == (dst[1], dst[0], 3) and got.dtype == np.uint8
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    assert np.array_equal(rgb, keep)


def test_anchors(built):
    import tiny_renderer_amd as T
    rng = np.random.default_rng(11)
    for f in (2, 4, 8):
        rgb = rng.integers(0, 256, (3 * f, 5 * f, 3), dtype=np.uint8)
        rgb[:f, :f] = 255
        assert np.array_equal(T.resize_host(rgb, 5, 3, "area"), RC.box(rgb, f)), f
    rgb = rng.integers(0, 256, (19, 23, 3), dtype=np.uint8)
    for filt in RC.FILTERS:
        assert np.array_equal(T.resize_host(rgb, 23, 19, filt), rgb), "the same size is a copy"
        # white stays white at the largest tap configuration; resize_np asserts its accumulators stay below 2^32
        white = np.full((9, 8192, 3), 255, np.uint8)
        for w, h in ((1024, 3), (1025, 3)):
            got = T.resize_host(white, w, h, filt)
            assert (got == 255).all() and np.array_equal(got, RC.resize_np(white, w, h, filt)), (filt, w, h)
        grey = np.full((9, 31, 3), 77, np.uint8)
        assert (T.resize_host(grey, 50, 4, filt) == 77).all(), "a constant frame stays constant"


def test_the_tile_cases_of_the_gpu_test_reach_every_shape(built):
    """tests/test_resize.py's outputs one past a multiple of every compiled tile: each runs in the shape it is meant for,
    by the rule written beside the shapes, under both filters."""
    for (w, h), shape in RC.TILE_CASES:
        tw, th = RC.TILES[shape]
        assert w % tw == 1 and h % th == 1
        for filt in RC.FILTERS:
            assert RC.shape_of(filt, 200, h) == shape, (w, h, filt)
    # and the last shape fits the worst vertical tables
    for n, m in ((8192, 1024), (8191, 1024), (488, 61), (200, 25)):
        assert RC.shape_of("bilinear", n, m) == 2 and RC.shape_of("area", n, m) is not None


def test_refusals_name_the_call_and_leave_out_alone(built):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    text = lambda: L.tr_last_error().decode()
    rgb = np.random.default_rng(5).integers(0, 256, (40, 64, 3), dtype=np.uint8)
    out = np.full((400, 600, 3), 0xAA, np.uint8)
    shrinks = ": a side shrinks by more than 8 (width and height must be at least an eighth of the source's, rounded up)"
    size = ": width and height must be 1..8192"
    filt = ": filter must be TR_RESIZE_AREA or TR_RESIZE_BILINEAR"
    cases = (((7, 5, 0, 0), shrinks), ((8, 4, 0, 0), shrinks), ((0, 5, 0, 0), size), ((8, 0, 1, 0), size), ((8193, 5, 0, 0), size),
             ((8, 8193, 0, 0), size), ((8, 5, 2, 0), filt), ((8, 5, 0, 1), ": flags must be 0"))
    for fields, why in cases:
        p = T.ResizeParams(*fields)
        assert L.tr_resize_host(64, 40, rgb.ctypes.data, C.addressof(p), out.ctypes.data) == _lib.TR_E_INVALID, fields
        assert text() == "tr_resize_host" + why, fields
    ok = T.ResizeParams(8, 5, 0, 0)
    assert L.tr_resize_host(64, 40, rgb.ctypes.data, None, out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_resize_host: null argument"
    assert L.tr_resize_host(64, 40, rgb.ctypes.data, C.addressof(ok), rgb.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_resize_host: out is rgb (the sizes differ and a pixel reads its neighbours: not in place)"
    assert L.tr_resize_host(64, 40, None, C.addressof(ok), out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_resize_host: null argument"
    assert (out == 0xAA).all(), "a refused call wrote `out`"
    # the smallest allowed size is accepted: ceil(64 / 8) x ceil(40 / 8)
    assert L.tr_resize_host(64, 40, rgb.ctypes.data, C.addressof(ok), out.ctypes.data) == 0
    # the taps: the same limits
    a = np.full(8200, 0xAAAA, np.uint16)
    b = np.full(8200 * 16, 0xAAAA, np.uint16)
    for f, n, m in ((0, 64, 7), (1, 64, 0), (0, 64, 8193), (2, 64, 8), (0, 0, 8)):
        assert L.tr_resize_taps(f, n, m, a.ctypes.data, a.ctypes.data, b.ctypes.data) == _lib.TR_E_INVALID and text().startswith("tr_resize_taps: ")
    assert L.tr_resize_taps(0, 64, 8, None, a.ctypes.data, b.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_resize_taps: null argument"
    assert (a == 0xAAAA).all() and (b == 0xAAAA).all()
    # Python refuses the same in the library's words
    for kw, why in ((dict(width=7, height=5), shrinks), (dict(width=0, height=5), size), (dict(width=8, height=5, filter="cubic"), filt)):
        with pytest.raises(ValueError) as e:
            T.resize_host(rgb, **kw)
        assert str(e.value) == "tr_resize_host" + why
