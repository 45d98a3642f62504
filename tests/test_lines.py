"""Lines on the device: tr_scene_lines / tr_scene_get_lined (k_lines) equal tr_lines_host in every byte.

Every comparison is np.array_equal against lines_host of what the scene itself returns (get_frame_buffer, read_z_f32);
tests/test_lines_host.py pins lines_host against the rule in numpy and asserts, on the oracle's frames of these very
cases, that the depth test rejects and passes candidates, that pixels have several survivors and that keys tie."""
import ctypes as C

import numpy as np
import pytest

from tests import lines_cases as LN
from tests import test_composite as TC
from tests import test_outline as TO

scene, snap, clean_flags, tiles_any = TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
other_synthetic = TC.other_synthetic
device_buffer, state, same_state, box = TO.device_buffer, TO.state, TO.same_state, TO.box
GUARD = 64
IDS = ["%dx%d" % s for s in LN.GPU_SIZES]


def drive(s, cam=LN.CAM, light=LN.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def keywords(combo):
    w, test, painter, opacity, bias = combo
    return dict(width=w, opacity=opacity, depth_test=test, painter=painter, depth_bias=bias)


def host(f, lines, kw):
    import tiny_renderer_amd as T
    return T.lines_host(f["fb"], f["z"], lines, T.lines_params(**kw))


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def table_of(T, rows, colour=(255, 255, 255, 255)):
    """rows of (x0, y0, z0, x1, y1, z1)."""
    r = np.asarray(rows, np.float64).reshape(-1, 6)
    return T.lines_table(r[:, 0:2].astype(np.int64), r[:, 2], r[:, 3:5].astype(np.int64), r[:, 5], colour)


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", LN.GPU_SIZES, ids=IDS)
def test_lined_frame_equals_the_host_rule_in_all_four_forms(small_synthetic, W, Hh):
    """Width 1, 2, 3 and 15, with and without the test, PAINTER: through the getter, into device memory, into a
    tr_host_alloc block and in place.  Out of place leaves the frame and its flags; in place leaves z, winner words and
    (test_what_stays) the shadow buffer."""
    s = scene(W, Hh, small_synthetic, "phong", LN.table(W, Hh), tap=True)
    lines = LN.segments(W, Hh)
    s.set_lines(lines)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    pinned = s.pinned_frame()
    for combo in LN.COMBOS:
        kw = keywords(combo)
        want = host(f, lines, kw)
        assert not np.array_equal(want, f["fb"])
        same(s.get_lined(**kw), want, "getter %r" % (kw,))
        dev = device_buffer(W * Hh * 3, 0xAB)
        pinned[...] = 0xAB
        s.lines(out=dev.data_ptr(), **kw)
        s.lines(out=pinned, **kw)
        assert s.sync() == 0
        same(dev.cpu().numpy().reshape(Hh, W, 3), want, "device memory %r" % (kw,))
        same(pinned, want, "tr_host_alloc %r" % (kw,))
        assert np.array_equal(clean_flags(s), flags), "an out-of-place call changed the frame's flags"
        same(s.get_frame_buffer(), f["fb"], "out of place leaves the scene's frame")
        s.lines(**kw)
        same(s.get_frame_buffer(), want, "in place %r" % (kw,))
        same_state(state(s), before)
        drive(s)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(256, 48), (131, 19)], ids=["words", "bytes"])
def test_out_at_an_odd_byte_offset_between_guards(small_synthetic, W, Hh):
    import torch
    s = scene(W, Hh, small_synthetic, "specular", LN.table(W, Hh))
    lines = LN.segments(W, Hh, seed=5)
    s.set_lines(lines)
    drive(s)
    f = snap(s)
    n = W * Hh * 3
    for kw in (keywords(LN.COMBOS[1]), keywords(LN.COMBOS[4])):
        want = host(f, lines, kw)
        for off in (1, 2, 3):
            out = torch.full((n + 2 * GUARD + off,), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert out.data_ptr() % 4 == 0
            s.lines(out=out.data_ptr() + GUARD + off, **kw)
            assert s.sync() == 0
            raw = out.cpu().numpy()
            same(raw[GUARD + off:GUARD + off + n].reshape(Hh, W, 3), want, "out + %d" % off)
            assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
        out = torch.full((Hh, W, 3), 0xAA, dtype=torch.uint8, device="cuda")
        s.lines(out=out, **kw)
        assert s.sync() == 0
        same(out.cpu().numpy(), want, "a tensor")
    same(s.get_frame_buffer(), f["fb"], "out of place leaves the scene's frame")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", ["phong", "shadow"])
def test_what_stays_and_which_flags_come_down(small_synthetic, pipe):
    """384 x 48: a flagged tile that no line reaches stays flagged and untouched; one a line enters is lowered and is
    zeros elsewhere; one whose only candidates get no winner (alpha or not: hidden behind nothing -- off-frame steps)
    stays flagged."""
    import tiny_renderer_amd as T
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, pipe, LN.table(W, Hh), tap=True)
    drive(s)
    f, before, flags = snap(s), state(s), clean_flags(s)
    assert flags.any() and not flags.all(), "flagged and unflagged tiles"
    ty, tx = np.argwhere(flags)[0]
    others = np.argwhere(flags)[1:]
    x0, y0 = int(tx) * 128, int(ty) * 16
    # one short segment inside the first flagged tile, and one that is binned there (width 15 reaches it) but at width 1
    # has no pixel in it: the tile below or above
    lines = table_of(T, [(x0 + 10, y0 + 5, 50.0, x0 + 40, y0 + 9, 60.0)], (200, 100, 50, 255))
    s.set_lines(lines)
    drive(s)
    s.lines(width=1)
    want = host(f, lines, dict(width=1))
    same(s.get_frame_buffer(), want, "in place")
    after = clean_flags(s)
    assert not after[ty, tx], "the flag of the tile the line entered came down"
    expect = flags.copy()
    expect[ty, tx] = False
    assert np.array_equal(after, expect), "only that flag changed"
    tile = want[::-1][y0:y0 + 16, x0:x0 + 128]
    assert tile.any() and int(tile.any(-1).sum()) == 31, "zeros elsewhere in the lowered tile"
    same_state(state(s), before)
    if len(others):
        # a neighbouring flagged tile in whose list the segment lies at width 15 only: no winner at width 1, the flag stays
        oy, ox = others[0]
        edge = table_of(T, [(int(ox) * 128 + 3, int(oy) * 16 + (18 if oy + 1 < 3 else -3), 50.0, int(ox) * 128 + 30, int(oy) * 16 + (18 if oy + 1 < 3 else -3), 50.0)])
        s.set_lines(edge)
        tiles, entries = s.debug_line_bins()
        assert entries >= 2, "the segment is listed in the tile it only reaches at width 15"
        drive(s)
        flags2 = clean_flags(s)
        s.lines(width=1)
        same(s.get_frame_buffer(), host(f, edge, dict(width=1)), "in place, a listed tile without a winner")
        after = clean_flags(s)
        assert after[oy, ox] == flags2[oy, ox], "a listed tile without a winner keeps its flag"
    s.close()


@pytest.mark.gpu
def test_a_cleared_scene_with_lines_as_wire_only_draws_them(small_synthetic):
    """--wire-only's sequence: render (for the depth), read nothing back, clear, then draw the lines without the test into
    the logically cleared frame."""
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", LN.table(W, Hh))
    lines = LN.segments(W, Hh, seed=21)
    s.set_lines(lines)
    drive(s)
    s.clear()
    black ={"fb": np.zeros((Hh, W, 3), np.uint8), "z": np.full((Hh, W), LN.F32_MIN, np.float32)}
    for kw in (dict(width=1, depth_test=False), dict(width=3, depth_test=True)):
        want = host(black, lines, kw)
        assert want.any()
        same(s.get_lined(**kw), want, "getter on a cleared scene")
        s.lines(**kw)
        same(s.get_frame_buffer(), want, "in place on a cleared scene")
        s.clear()
    # nothing to draw: the cleared shortcut (zeros out of place, nothing in place)
    dev = device_buffer(W * Hh * 3, 0xAB)
    s.lines(opacity=0, out=dev.data_ptr())
    s.lines(opacity=0)
    assert s.sync() == 0 and not dev.cpu().numpy().any() and not s.get_frame_buffer().any()
    s.close()


@pytest.mark.gpu
def test_transient_depth_stays_transient_without_the_test(small_synthetic):
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", LN.table(W, Hh), auto_group=False)
    s.set_lines(LN.segments(W, Hh))
    out = device_buffer(W * Hh * 3)
    s.profile_enable(True)
    drive(s)
    s.lines(width=2, depth_test=False, out=out.data_ptr())
    s.lines(width=2, depth_test=False)
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof["k_tile"]["launches"] == 1 and prof.get("k_tile_depth", {}).get("launches", 0) == 0, "lines repeated the pass for a depth they do not read: %r" % (prof,)
    assert prof.get("k_lines", {}).get("launches") == 2 and prof["k_lines"]["total_ms"] > 0.0, prof
    s.lines(width=2)
    assert s.sync() == 0
    prof = s.profile_read()
    tiles = prof["k_tile"]["launches"] + prof.get("k_tile_depth", {}).get("launches", 0)
    assert tiles == 2, "the depth was not transient: the case shows nothing (%r)" % (prof,)
    s.close()


@pytest.mark.gpu
def test_a_tile_with_3000_segments(small_synthetic):
    """The walk goes far beyond one round of the workgroup's four waves."""
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    rng = np.random.default_rng(30)
    n = 3000
    xy0 = np.stack([rng.integers(128, 256, n), rng.integers(16, 32, n)], 1)
    xy1 = np.stack([rng.integers(128, 256, n), rng.integers(16, 32, n)], 1)
    lines = T.lines_table(xy0, rng.random(n) * 100.0, xy1, rng.random(n) * 100.0, rng.integers(0, 256, (n, 4)))
    s = scene(W, Hh, small_synthetic, "phong", LN.table(W, Hh))
    s.set_lines(lines)
    tiles, entries = s.debug_line_bins()
    assert entries >= n and tiles <= 9
    drive(s)
    f = snap(s)
    for kw in (dict(width=1), dict(width=2, depth_test=False), dict(width=1, painter=True, depth_test=False)):
        same(s.get_lined(**kw), host(f, lines, kw), "%r" % (kw,))
    s.lines(width=1)
    same(s.get_frame_buffer(), host(f, lines, dict(width=1)), "in place")
    s.close()


@pytest.mark.gpu
def test_one_segment_across_all_tiles_is_binned_by_the_tiles_it_crosses(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 1024, 128
    s = scene(W, Hh, small_synthetic, "phong", store_depth=True)
    lines = table_of(T, [(0, 0, 10.0, W - 1, Hh - 1, 90.0)], (250, 240, 10, 255))
    s.set_lines(lines)
    x, y, _ = LN.candidates(lines[0], 1, 0.0, W, Hh)
    crossed = len(set(zip((y // 16).tolist(), (x // 128).tolist())))
    tiles, entries = s.debug_line_bins()
    assert tiles == entries and crossed <= entries <= 2 * crossed < 64, "%d entries, %d tiles crossed" % (entries, crossed)
    drive(s)
    f = snap(s)
    for kw in (dict(width=1), dict(width=15, depth_test=False)):
        same(s.get_lined(**kw), host(f, lines, kw), "%r" % (kw,))
    s.lines(width=15)
    same(s.get_frame_buffer(), host(f, lines, dict(width=15)), "in place")
    s.close()


@pytest.mark.gpu
def test_no_segments_segments_off_the_frame_and_a_second_table(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 200, 40
    s = scene(W, Hh, small_synthetic, "phong", LN.table(W, Hh))
    drive(s)
    f, flags = snap(s), clean_flags(s)
    p = T.lines_params()
    host_out = np.full((Hh, W, 3), 0xAA, np.uint8)
    # no table: refused, by both entry points, before anything else
    for who, call in (("tr_scene_lines", lambda: L.tr_scene_lines(s._h, C.addressof(p), None)),
                      ("tr_scene_get_lined", lambda: L.tr_scene_get_lined(s._h, C.addressof(p), host_out.ctypes.data))):
        assert call() == _lib.TR_E_INVALID and L.tr_last_error().decode() == who + ": the scene has no table of lines (tr_scene_set_lines)"
    assert s.debug_line_bins() == (0, 0)
    # every segment off the frame: a table, but nothing to draw
    off = table_of(T, [(-50, -50, 1.0, -10, 300, 2.0), (W + 9, 0, 1.0, W + 40, Hh, 2.0), (0, Hh + 8, 1.0, W, Hh + 8, 1.0)])
    s.set_lines(off)
    assert s.debug_line_bins() == (0, 0)
    same(s.get_lined(width=15), f["fb"], "off the frame, getter")
    dev = device_buffer(W * Hh * 3, 0xAB)
    s.lines(width=15, out=dev.data_ptr())
    s.lines(width=15)
    assert s.sync() == 0
    same(dev.cpu().numpy().reshape(Hh, W, 3), f["fb"], "off the frame, out of place: a copy")
    same(s.get_frame_buffer(), f["fb"], "off the frame, in place")
    assert np.array_equal(clean_flags(s), flags)
    # set_lines twice between two calls: the second table is used
    a, b = LN.segments(W, Hh, 40, seed=1), LN.segments(W, Hh, 50, seed=2)
    s.set_lines(a)
    first = s.get_lined(width=2)
    s.set_lines(a), s.set_lines(b)
    second = s.get_lined(width=2)
    same(first, host(f, a, dict(width=2)), "the first table")
    same(second, host(f, b, dict(width=2)), "the second table")
    assert not np.array_equal(first, second)
    # n == 0 drops the table; a refused table leaves the old one
    bad = a.copy()
    bad["x0"][3] = (1 << 20) + 1
    with pytest.raises(Exception) as e:
        s.set_lines(bad)
    assert "tr_scene_set_lines: segment 3: coordinates must lie within +-2^20" in str(e.value)
    same(s.get_lined(width=2), second, "a refused table leaves the old one")
    s.set_lines(None)
    assert L.tr_scene_lines(s._h, C.addressof(p), None) == _lib.TR_E_INVALID
    # the refusals in their order: no table, then a band scene; parameters first of all
    band = scene(256, 48, small_synthetic, "phong", LN.table(256, 48), band_rows=(16, 32))
    assert L.tr_scene_lines(band._h, C.addressof(p), None) == _lib.TR_E_INVALID
    assert L.tr_last_error().decode() == "tr_scene_lines: the scene has no table of lines (tr_scene_set_lines)"
    badp = T.LinesParams(0, 256, 1, 0.0, (C.c_uint32 * 4)())
    assert L.tr_scene_lines(band._h, C.addressof(badp), None) == _lib.TR_E_INVALID and L.tr_last_error().decode() == "tr_scene_lines: width must be 1..15"
    s.set_lines(a)
    assert L.tr_scene_lines(s._h, C.addressof(p), host_out.ctypes.data) == _lib.TR_E_INVALID
    assert L.tr_last_error().decode() == "tr_scene_lines: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_lined takes any host memory)"
    assert L.tr_scene_lines(s._h, C.addressof(p), int(s.band_tiles().frame_buffer_device) + 3) == _lib.TR_E_INVALID
    assert L.tr_last_error().decode() == "tr_scene_lines: `out` overlaps a frame buffer of the scene (out == NULL draws in place)"
    assert (host_out == 0xAA).all()
    same(s.get_frame_buffer(), f["fb"], "a refused call changed the frame")
    s.close(), band.close()


@pytest.mark.gpu
def test_a_wireframe_at_bias_0_hides_every_pixel_of_the_far_side(small_synthetic):
    """wireframe_lines of the procedural mesh under the depth test at bias 0: a pixel the device draws is a pixel where
    the edge is not behind the surface -- shown as an image property against lines_host: the device equals the host rule,
    and under the host rule no pixel that only far-side edges cover (every candidate there has zl <= zbuf) changes."""
    import tiny_renderer_amd as T
    W, Hh = 200, 120
    s = scene(W, Hh, small_synthetic, "phong", store_depth=True)
    drive(s)
    f = snap(s)
    lines = T.wireframe_lines(s, small_synthetic[0], (255, 0, 255, 255))
    assert lines.shape[0] == T.mesh_edges(small_synthetic[0]).shape[0] > 100
    s.set_lines(lines)
    tested, xray = s.get_lined(width=1), s.get_lined(width=1, depth_test=False)
    same(tested, host(f, lines, dict(width=1)), "tested")
    same(xray, host(f, lines, dict(width=1, depth_test=False)), "x-ray")
    census = {}
    LN.winners(f["z"], lines, 1, True, False, 0.0, census=census)
    hidden = ((census["survivors"] == 0) & (census["rejected"] > 0))[::-1]
    assert hidden.any(), "no pixel is covered by hidden edges only: the case shows nothing"
    assert np.array_equal(tested[hidden], f["fb"][hidden]), "a pixel of an edge behind the surface was drawn"
    assert (xray[hidden] == (255, 0, 255)).all(), "x-ray draws them"
    assert int((tested != f["fb"]).any(-1).sum()) < int((xray != f["fb"]).any(-1).sum())
    s.close()


@pytest.mark.gpu
def test_consumers_see_the_lines(small_synthetic, other_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", LN.table(W, Hh))
    lines = LN.segments(W, Hh, seed=8)
    lines["rgba"][:, 3] = 255
    s.set_lines(lines)
    drive(s)
    f = snap(s)
    want = host(f, lines, dict(width=3, depth_bias=1.0))
    s.lines(width=3, depth_bias=1.0)
    same(s.resolve(2), box(want, 2), "resolve by 2 after lines in place")
    dst = scene(W, Hh, other_synthetic, "phong")
    drive(dst, cam=1.1)
    d = snap(dst)
    dst.composite(s)
    zc, fc = T.composite_host(d["z"][::-1], d["fb"], f["z"][::-1], want)
    assert not np.array_equal(fc, T.composite_host(d["z"][::-1], d["fb"], f["z"][::-1], f["fb"])[1]), "no line pixel wins the merge"
    same(dst.get_frame_buffer(), fc, "composite into a second scene after lines in place")
    s.close(), dst.close()
