"""Frame statistics on the device: tr_scene_frame_stats / tr_scene_get_frame_stats (k_stats, k_stats_finish).

Every comparison is whole-record equality (all 6192 bytes) against tr_frame_stats_host of a snapshot -- get_frame_buffer()
and read_z_f32() -- of the very frame, which is then rendered again so that its fast-clear flags are fresh and its depth,
without TR_OPT_STORE_DEPTH, is back on the chip.  tests/test_frame_stats_host.py pins the host rule against numpy.  Every
case first asserts ON THE EXPECTATION that it is not vacuous."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import test_composite as TC
from tests import test_grade as TG

bits, drive, scene, snap, clean_flags, tiles_any = TC.bits, TC.drive, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
PIPE, AT, CORNER_AT = TG.PIPE, TG.AT, TG.CORNER_AT
F32_MIN_BITS = np.uint32(0xFF7FFFFF)
# 130 x 17 has 2 x 2 tiles: the right column two pixels wide, the upper row one row high.  Candidate places for a small
# model across the right edge; the test takes the first under which a two-column tile is drawn into and another is flagged.
SMALL_AT = np.array([[-0.5, 0.0, 0.0, 0.3]], np.float32)          # 256 x 48: the model inside the left tile column
EDGE_PLACES = [np.array([[x, y, 0.0, r]], np.float32) for r in (0.3, 0.2, 0.45) for x in (0.95, 0.85, 1.05) for y in (-0.3, 0.0, -0.6)]


def zrange(f):
    """z_lo and z_scale that spread the snapshot's drawn depths over some 200 bins."""
    z = f["z"][bits(f["z"]) != F32_MIN_BITS]
    assert z.size > 16 and np.isfinite(z).all() and z.max() > z.min()
    return dict(z_lo=float(z.min()), z_scale=float(np.float32(200.0) / (z.max() - z.min())))


def host(f, depth, window=None, zkw=None):
    import tiny_renderer_amd as T
    return T.frame_stats_host(f["fb"], f["z"] if depth else None, window=window, depth=depth, **(zkw if depth else {}))


def telling(st, depth):
    """The expectation is not vacuous: colours beside black, and with depth a histogram over many bins."""
    assert st.n_pixels > 0
    if depth:
        assert 0 < st.n_drawn < st.n_pixels and (st.zhist != 0).sum() >= 8, "the depth histogram shows nothing: %r" % (st,)
        assert st.box[2] > st.box[0] and st.box[3] > st.box[1]
    assert (st.luma != 0).sum() >= 8 and st.luma[0] > 0, "the frame is flat"


def diff(got, want):
    return "%r != %r (%d words differ)" % (got, want, int((got.raw.view(np.uint32) != want.raw.view(np.uint32)).sum()))


def check(s, f, depth, window=None, zkw=None, redraw=True, want=None, **drive_kw):
    """The getter's record of scene s against the host rule over snapshot f."""
    want = host(f, depth, window, zkw) if want is None else want
    if redraw:
        drive(s, **drive_kw)
    got = s.get_frame_stats(window=window, depth=depth, **(zkw if depth else {}))
    assert got == want, diff(got, want)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("store_depth", [False, True])
@pytest.mark.parametrize("W,Hh", [(128, 16), (130, 17), (256, 48), (500, 300), (512, 512)])
def test_record_equals_the_host_rule(small_synthetic, W, Hh, store_depth):
    """128 x 16: one tile; 130 x 17: partial tiles on both axes, guarded bytes, a tile column of two pixels; 256 x 48 and
    512 x 512: whole words; 500 x 300: ragged on both axes, whole words.  Colour only and with depth; with the depth stored
    and left on the chip -- the two scenes' records must be the same."""
    at = SMALL_AT if (W, Hh) == (256, 48) else AT
    if (W, Hh) == (130, 17):
        at = None
        for cand in EDGE_PLACES:
            s = scene(W, Hh, small_synthetic, PIPE, cand, store_depth=store_depth, auto_group=False)
            drive(s)
            fb, flags = s.get_frame_buffer(), clean_flags(s)
            s.close()
            if flags.shape == (2, 2) and flags[:, 1].any() and not flags[:, 1].all() and (fb[:, 128:] != 0).any():
                at = cand
                break
        assert at is not None, "no place gives a flagged edge tile of 2 columns beside a drawn one"
    s = scene(W, Hh, small_synthetic, PIPE, at, store_depth=store_depth, auto_group=False)
    drive(s)
    f, flags = snap(s), clean_flags(s)
    if (W, Hh) != (128, 16):
        assert flags.any() and not flags.all(), "the frame needs flagged tiles and drawn ones"
    zkw = zrange(f)
    telling(check(s, f, False), False)
    telling(check(s, f, True, zkw=zkw), True)
    # the other scene's snapshot gives the same records: the rule sees the frame, not how its depth is kept
    o = scene(W, Hh, small_synthetic, PIPE, at, store_depth=not store_depth, auto_group=False)
    check(o, f, True, zkw=zkw)
    o.close()
    if not store_depth:
        # colour-only statistics leave the depth on the chip: no depth-only repeat of the pass (tests/test_bloom.py's observable)
        s.profile_enable(True)
        drive(s)
        check(s, f, False, redraw=False)
        s.frame_stats()
        assert s.sync() == 0
        prof = s.profile_read()
        assert prof["k_tile"]["launches"] == 1, "colour statistics repeated the pass for its depth: %r" % (prof,)
        assert prof.get("k_stats", {}).get("launches") == 2 and prof["k_stats"]["total_ms"] > 0.0, prof
        check(s, f, True, zkw=zkw, redraw=False)
        assert s.profile_read()["k_tile"]["launches"] == 2, "the depth was not transient: the case shows nothing"
    s.close()


@pytest.mark.gpu
def test_windows(small_synthetic):
    W, Hh = 384, 48
    s = scene(W, Hh, small_synthetic, PIPE, CORNER_AT, store_depth=True)
    drive(s)
    f, flags = snap(s), clean_flags(s)
    zkw = zrange(f)
    drawn = bits(f["z"]) != F32_MIN_BITS
    assert flags.shape == (3, 3) and flags[:, 0].all() and not flags[1, 2], "left tile column flagged, the model in the right one"
    ys, xs = np.nonzero(drawn[::-1])                                   # output rows
    cx, cy = int(np.median(xs)), int(np.median(ys))
    # a rectangle of drawn pixels inside one drawn tile
    j = next(j for j in range(3) if not flags[j, 2])
    wins = {"whole": None,
            "one pixel, drawn": (cx, cy, 1, 1),
            "one pixel, in a flagged tile": (5, 20, 1, 1),
            "an edge inside a tile": (256 + 30, 3, 50, 7),
            "across tile borders on both axes": (100, 10, 200, 30),
            "wholly in flagged tiles": (3, 2, 120, 44),
            "wholly in one drawn tile": (256, Hh - 16 * (j + 1), 128, 16),
            "odd edges": (257, 1, 126, 46),
            "one column": (cx, 0, 1, Hh),
            "one row": (0, cy, W, 1)}
    for name, win in wins.items():
        want = check(s, f, True, win, zkw)
        check(s, f, False, win)
        x0, y0, w, h = win if win else (0, 0, W, Hh)
        assert want.n_pixels == w * h, name
        if name == "wholly in flagged tiles" or name == "one pixel, in a flagged tile":
            assert want.n_drawn == 0 and want.luma[0] == want.n_pixels and want.box == (0, 0, 0, 0), name
        if name in ("one pixel, drawn", "wholly in one drawn tile", "one column", "one row", "across tile borders on both axes"):
            assert want.n_drawn > 0, name
            assert x0 <= want.box[0] < want.box[2] <= x0 + w and y0 <= want.box[1] < want.box[3] <= y0 + h, name
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(256, 48), (512, 512)])
def test_the_walk_under_a_cap(small_synthetic, W, Hh):
    """Caps of 1, 2, 3 and 7 workgroups: each walks several tiles (6 and 128 of them) and k_stats_finish sums that many
    slots; the record is the uncapped one."""
    n_tiles = ((W + 127) // 128) * ((Hh + 15) // 16)
    s = scene(W, Hh, small_synthetic, PIPE, SMALL_AT if W == 256 else AT, store_depth=True)
    assert s.debug_stats_grid(0) == 0, "no k_stats launch yet"
    drive(s)
    f = snap(s)
    zkw = zrange(f)
    want = check(s, f, True, zkw=zkw)
    telling(want, True)
    free = s.debug_stats_grid(0)
    assert 0 < free <= n_tiles
    win = (W // 3, Hh // 4, W // 2, Hh // 2)
    for cap in (1, 2, 3, 7):
        s.debug_stats_grid(cap)
        for depth in (False, True):
            check(s, f, depth, zkw=zkw)
            assert s.debug_stats_grid(cap) == min(cap, free), "cap %d" % cap
            check(s, f, depth, win, zkw)
    s.debug_stats_grid(0)
    check(s, f, True, zkw=zkw, want=want)
    assert s.debug_stats_grid(0) == free
    s.close()


@pytest.mark.gpu
def test_flat_and_non_black_frames_after_the_other_stages(small_synthetic, other_synthetic):
    import tiny_renderer_amd as T
    from tests import test_bloom as TB
    from tests import test_depth_of_field as TD
    W, Hh = 384, 48
    at = TC._small(-0.4, 0.1)
    ref = scene(W, Hh, small_synthetic, PIPE, at, store_depth=True)
    drive(ref)
    f, flags = snap(ref), clean_flags(ref)
    ref.close()
    assert flags.any() and not flags.all()
    zkw = zrange(f)

    def after(fb):
        return dict(f, fb=fb)

    # graded in place by a constant table that is not black: flags come down, every pixel one colour
    lut = np.empty((2, 2, 2, 3), np.uint8)
    lut[...] = (9, 200, 77)
    flat = T.grade_host(f["fb"], lut)
    assert (flat == (9, 200, 77)).all()
    s = scene(W, Hh, small_synthetic, PIPE, at, store_depth=True)
    s.set_lut(lut)
    for cap in (0, 2):
        s.debug_stats_grid(cap)
        drive(s), s.grade()
        assert not clean_flags(s).any(), "the flags did not follow the grade"
        want = host(after(flat), True, zkw=zkw)
        assert want.hist[0][9] == W * Hh and want.hist[1][200] == W * Hh and want.max_channel[200] == W * Hh
        check(s, after(flat), True, zkw=zkw, redraw=False, want=want)
        check(s, after(flat), False, (100, 10, 57, 30), redraw=False)
    s.debug_stats_grid(0)
    # a graded frame that is not flat: a random table with a non-black entry 0
    lut = TG.lut_c0(9, (3, 0, 250), 11)
    drive(s), s.set_lut(lut), drive(s), s.grade()
    check(s, after(T.grade_host(f["fb"], lut)), True, zkw=zkw, redraw=False)
    s.set_lut(None)
    # bloom, depth of field and ambient occlusion in place
    bp = TB.P(8, TB.mid_threshold(f["fb"]), 512)
    bloomed = TB.expectation(f["fb"], bp)
    drive(s), s.bloom(bp)
    assert not (clean_flags(s) & tiles_any(bloomed[::-1].any(-1))).any(), "a tile with colour in it is flagged clean"
    telling(check(s, after(bloomed), True, zkw=zkw, redraw=False), True)
    dp = TD.params_for(f, 3)
    soft = T.depth_of_field_host(f["z"], f["fb"], dp)
    assert not np.array_equal(soft, f["fb"])
    drive(s), s.depth_of_field(dp)
    check(s, after(soft), True, zkw=zkw, redraw=False)
    shaded = T.ambient_occlusion_host(f["z"], f["fb"], radius=8, rings=2)
    assert not np.array_equal(shaded, f["fb"])
    drive(s), s.ambient_occlusion(radius=8, rings=2)
    check(s, after(shaded), True, zkw=zkw, redraw=False)
    # composite: another model merged in -- colour, depth and both kinds of flags change
    o = scene(W, Hh, other_synthetic, PIPE, TC._small(-0.2, 0.0, 0.2), store_depth=True)
    drive(o, light=0.2)
    fo = snap(o)
    merged, wins = TC.merge(f, fo)
    assert wins.any() and not wins.all()
    drive(s), drive(o, light=0.2)
    s.composite(o)
    mkw = zrange(merged)
    want = check(s, merged, True, zkw=mkw, redraw=False)
    assert want.n_drawn > host(f, True, zkw=mkw).n_drawn
    s.close(), o.close()


@pytest.mark.gpu
def test_a_callers_buffer_a_kept_frame_and_a_cleared_scene(small_synthetic):
    import torch
    W, Hh = 256, 48
    # a caller's buffer of random bytes, not trusted, rendered into without a clear: the backdrop is counted as it is
    nb = W * Hh * 3
    noise = np.random.default_rng(5).integers(0, 256, nb, dtype=np.uint8)
    buf = torch.from_numpy(noise.copy()).cuda()
    torch.cuda.synchronize()
    d = scene(W, Hh, small_synthetic, PIPE, AT, store_depth=True)
    d.set_frame_buffer_device(buf.data_ptr())
    drive(d, clear=False)
    got = {depth: d.get_frame_stats(depth=depth, z_lo=0.0, z_scale=1.0) for depth in (False, True)}
    f = snap(d)
    assert not np.array_equal(f["fb"].reshape(-1), noise), "nothing was drawn over the noise"
    assert len(np.unique(f["fb"].reshape(-1, 3), axis=0)) > nb // 6, "the frame is not noise"
    for depth in (False, True):
        want = host(f, depth, zkw=dict(z_lo=0.0, z_scale=1.0))
        assert got[depth] == want, diff(got[depth], want)
    assert (got[False].hist != 0).all(axis=1).sum() >= 3, "noise fills every bin of the channels"
    assert np.array_equal(buf.cpu().numpy().reshape(Hh, W, 3), f["fb"]), "the statistics wrote the caller's buffer"
    d.close()
    # a kept frame chosen with select_frame
    par = TC._params(4)
    kept = []
    for twin in (True, False):
        g = scene(W, Hh, small_synthetic, PIPE, AT, frames_per_launch=4)
        g.render_frames(par)
        assert g.frames_kept() >= 3
        if twin:
            for back in range(3):
                g.select_frame(back)
                kept.append(snap(g))
            assert not np.array_equal(kept[0]["fb"], kept[1]["fb"])
        else:
            for back in (1, 0, 2):
                g.select_frame(back)
                zkw = zrange(kept[back])
                want = check(g, kept[back], True, zkw=zkw, redraw=False)
                check(g, kept[back], False, redraw=False)
            assert host(kept[0], True, zkw=zkw) != host(kept[1], True, zkw=zkw), "the kept frames' records do not differ"
        g.close()
    # logically cleared: a black frame in which nothing is drawn; the pending clear stays pending
    s = scene(W, Hh, small_synthetic, PIPE, AT)
    drive(s)
    s.clear()
    black = {"fb": np.zeros((Hh, W, 3), np.uint8), "z": np.full((Hh, W), TC.F32_MIN, np.float32)}
    for win in (None, (100, 7, 60, 30)):
        want = check(s, black, True, win, dict(z_lo=0.0, z_scale=1.0), redraw=False)
        n = W * Hh if win is None else win[2] * win[3]
        assert (want.hist[:, 0] == n).all() and want.n_drawn == 0 and want.n_pixels == n
        check(s, black, False, win, redraw=False)
    assert not s.get_frame_buffer().any() and (bits(s.read_z_f32()) == F32_MIN_BITS).all()
    s.close()


@pytest.mark.gpu
def test_band_scenes_and_their_merge(small_synthetic):
    """640 x 96 in two bands that are not tile-aligned: rows [0, 40) and [40, 96)."""
    import tiny_renderer_amd as T
    W, Hh, cut = 640, 96, 40
    at = np.array([[-0.25, 0.0, 0.0, 0.7]], np.float32)
    whole = scene(W, Hh, small_synthetic, PIPE, at, store_depth=True)
    drive(whole)
    f = snap(whole)
    zkw = zrange(f)
    want_whole = check(whole, f, True, zkw=zkw)
    telling(want_whole, True)
    whole.close()
    records = []
    for band in ((0, cut), (cut, Hh)):
        b = scene(W, Hh, small_synthetic, PIPE, at, store_depth=True, band_rows=band)
        for cap in (0, 3):
            b.debug_stats_grid(cap)
            drive(b)
            got = b.get_frame_stats(depth=True, **zkw)
            want = host(f, True, (0, band[0], W, band[1] - band[0]), zkw)
            assert got == want, "band %r, cap %d: %s" % (band, cap, diff(got, want))
            assert got.n_pixels == W * (band[1] - band[0]) and got.n_drawn > 0
            # a window across the band's edge: only the band's rows take part
            win = (50, cut - 20, 400, 45)
            r0, r1 = max(win[1], band[0]), min(win[1] + win[3], band[1])
            got = b.get_frame_stats(window=win, depth=True, **zkw)
            want = host(f, True, (win[0], r0, win[2], r1 - r0), zkw)
            assert got == want, "band %r, window: %s" % (band, diff(got, want))
        records.append(b.get_frame_stats(depth=True, **zkw))
        b.close()
    assert T.frame_stats_merge(records[0], records[1]) == want_whole
    assert T.frame_stats_merge(records[1], records[0]) == want_whole


@pytest.mark.gpu
def test_out_kinds_agree_and_nothing_else_changes(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    from tiny_renderer_amd.scene import FRAME_STATS_BYTES, FrameStats
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, PIPE, AT, tap=True, store_depth=True)
    drive(s)
    f, flags = snap(s), clean_flags(s)
    zkw = zrange(f)
    want = host(f, True, zkw=zkw)
    other = host(f, True, (10, 5, 200, 30), zkw)
    assert other != want
    drive(s)
    dev = TG.device_buffer(FRAME_STATS_BYTES + 64)                     # 0xAB everywhere: a byte that is not written shows
    pinned = s.pinned_stats()
    pinned[:] = 0xAB
    for round_ in range(2):                                            # a second call overwrites, it does not accumulate
        s.frame_stats(depth=True, out=dev.data_ptr() + 16, **zkw)
        s.frame_stats(depth=True, out=pinned, **zkw)
        own = s.frame_stats(depth=True, **zkw)
        assert s.sync() == 0
        raw = dev.cpu().numpy()
        assert FrameStats(raw[16:16 + FRAME_STATS_BYTES]) == want, "device memory, round %d" % round_
        assert (raw[:16] == 0xAB).all() and (raw[16 + FRAME_STATS_BYTES:] == 0xAB).all(), "a guard byte changed"
        assert FrameStats(pinned) == want and FrameStats(own) == want, "page-locked memory, round %d" % round_
        assert s.get_frame_stats(depth=True, **zkw) == want
    # another window into the same buffers: nothing of the first record is left
    s.frame_stats(window=(10, 5, 200, 30), depth=True, out=pinned, **zkw)
    assert s.sync() == 0 and FrameStats(pinned) == other
    # ordered like tr_scene_resolve: a later render is behind it, held-back frames are ahead of it
    a = scene(W, Hh, small_synthetic, PIPE, AT, store_depth=True, auto_group=True)
    drive(a, cam=1.0), drive(a, cam=2.0), drive(a)
    a.frame_stats(depth=True, out=pinned, **zkw)
    drive(a, cam=1.0)
    assert a.sync() == 0 and FrameStats(pinned) == want
    a.close()
    # the frame, z, winner words and flags are what they were
    assert np.array_equal(clean_flags(s), flags), "the statistics changed the frame's flags"
    TC.same(snap(s), f)
    s.close()


@pytest.mark.gpu
def test_refusals_on_the_device_queue_nothing(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    from tiny_renderer_amd.scene import stats_params, FRAME_STATS_BYTES
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, PIPE, AT, tap=True)
    drive(s)
    f = snap(s)
    drive(s)
    pinned = s.pinned_stats()
    pinned[:] = 0xAB
    host_out = np.full(FRAME_STATS_BYTES, 0xAB, np.uint8)
    good = stats_params((1, 1, 30, 20), True, 0.0, 1.0)
    bad = [("struct_size", 28, b"struct_size"), ("flags", 2, b"unknown flags"), ("w", 0, b"window"), ("h", 0, b"window"),
           ("x0", W - 29, b"outside the frame"), ("y0", Hh - 19, b"outside the frame"), ("w", 0xFFFFFFFF, b"outside the frame"),
           ("z_lo", float("nan"), b"z_lo"), ("z_scale", 0.0, b"z_scale"), ("z_scale", float("inf"), b"z_scale")]
    for field, v, text in bad:
        q = stats_params((1, 1, 30, 20), True, 0.0, 1.0)
        setattr(q, field, v)
        assert L.tr_scene_frame_stats(s._h, C.addressof(q), pinned.ctypes.data) == _lib.TR_E_INVALID and text in L.tr_last_error(), (field, v)
        assert L.tr_scene_get_frame_stats(s._h, C.addressof(q), host_out.ctypes.data) == _lib.TR_E_INVALID and text in L.tr_last_error(), (field, v)
    assert L.tr_scene_frame_stats(s._h, None, pinned.ctypes.data) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_scene_frame_stats(s._h, C.addressof(good), None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    assert L.tr_scene_get_frame_stats(s._h, C.addressof(good), None) == _lib.TR_E_INVALID and b"null" in L.tr_last_error()
    plain = np.full(FRAME_STATS_BYTES, 0xAB, np.uint8)
    assert L.tr_scene_frame_stats(s._h, C.addressof(good), plain.ctypes.data) == _lib.TR_E_INVALID and b"tr_host_alloc" in L.tr_last_error()
    small = L.tr_host_alloc(FRAME_STATS_BYTES - 1)
    assert small
    assert L.tr_scene_frame_stats(s._h, C.addressof(good), small) == _lib.TR_E_INVALID and b"smaller" in L.tr_last_error()
    L.tr_host_free(small)
    with pytest.raises(T.TinyRendererError):
        s.frame_stats(out=plain)
    with pytest.raises(ValueError):
        s.frame_stats(out=np.zeros(100, np.uint8))
    assert s.sync() == 0
    assert (pinned == 0xAB).all() and (host_out == 0xAB).all() and (plain == 0xAB).all(), "a refused call wrote a record"
    assert s.debug_stats_grid(0) == 0, "a refused call launched k_stats"
    TC.same(snap(s), f)
    s.close()


@pytest.mark.gpu
def test_cli_auto_levels_autofocus_and_stats(small_synthetic, tmp_path, capsys):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    common = ["--synthetic", "-s", "phong", "--width", "256", "--height", "128", "--camera-angle", "0.3", "--light-angle", "0.7"]
    hd = b"P6\n256 128\n255\n"

    def run(name, *more):
        path = str(tmp_path / name)
        assert cli.main(common + list(more) + ["--out", path]) == 0
        return np.frombuffer(open(path, "rb").read()[len(hd):], np.uint8).reshape(128, 256, 3)

    plain = run("plain.ppm", "--stats")
    text = stats_text = capsys.readouterr().out
    st = T.frame_stats_host(plain)
    lo, mid, hi = (T.hist_percentile(st.luma, q) for q in (0.01, 0.5, 0.99))
    assert "stats --- pixels %d drawn " % (256 * 128) in text and "luma 1%% %d 50%% %d 99%% %d" % (lo, mid, hi) in text, text
    levelled = run("levels.ppm", "--auto-levels", "0.01,0.99")
    assert np.array_equal(levelled, T.grade_host(plain, T.lut_auto_levels(st, 0.01, 0.99)))
    st2 = T.frame_stats_host(levelled)
    lo2, hi2 = T.hist_percentile(st2.luma, 0.01), T.hist_percentile(st2.luma, 0.99)
    assert lo < hi < 255, "the plain picture's tones already span the range: the case shows nothing"
    assert lo2 <= lo and hi2 > hi, "the picture's own 1 %% / 99 %% bins did not move outward: %d, %d -> %d, %d" % (lo, hi, lo2, hi2)
    # autofocus: the focus it prints is depth_median's, and the picture is --dof-focus at that depth; a scale from the
    # depth range --stats printed, so that the far and the near parts are blurred
    import re
    zmin, zmax = (float(v) for v in re.search(r"z \[([^,]+), ([^\]]+)\]", stats_text).groups())
    assert zmax > zmin
    dof = ["--dof-scale", repr(8.0 / (zmax - zmin)), "--dof-radius", "6"]
    auto = run("auto.ppm", "--dof-autofocus", *dof)
    text = capsys.readouterr().out
    focus = float(text.split("autofocus --- z ")[1].split()[0])
    assert zmin < focus < zmax
    mesh, texs = T.synthetic_scene()
    s = T.Scene(256, 128, mesh, texs, "phong")
    drive_cli(s)
    assert T.depth_median(s, (64, 32, 128, 64)) == focus
    s.close()
    fixed = run("fixed.ppm", "--dof-focus=%r" % focus, *dof)
    assert np.array_equal(auto, fixed) and not np.array_equal(auto, plain)


def drive_cli(s):
    """The one frame the CLI renders under --camera-angle 0.3 --light-angle 0.7."""
    ca, la = np.float32(0.3), np.float32(0.7)
    s.clear()
    s.set_light_direction([float(np.sin(la)), 0.0, float(np.cos(la))])
    s.set_camera([float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0])
    s.render()


@pytest.fixture(scope="module")
def other_synthetic(built):
    import tiny_renderer_amd as T
    return T.synthetic_scene(n_lat=9, n_lon=17, tex_size=128, radius=0.75)
