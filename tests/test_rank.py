"""Rank on the device: tr_scene_rank / tr_scene_get_ranked (k_rank) equal tr_rank_host in every byte.

Every comparison is np.array_equal against rank_host of the frame the scene itself returns; tests/test_rank_host.py pins
rank_host against the rule in numpy.  Footprints, ranks, ops, edges and frame sizes are tests/rank_cases.py's."""
import ctypes as C

import numpy as np
import pytest

from tests import dense_cases as DC
from tests import helpers as H
from tests import rank_cases as RC
from tests import test_composite as TC
from tests import test_dense_frames as TD
from tests import test_outline as TO
from tests import test_resolve as TR

scene, snap, clean_flags = TC.scene, TC.snap, TC.clean_flags
device_buffer = TO.device_buffer
PIPELINES = TR.PIPELINES
GUARD = 64
ALL = RC.everything()
# both compiled selections, every op, the mirror-sensitive footprint, the largest box
SUBSET = ("3x3_rank4", "15x15_rank112", "15x15_rank0", "L_median", "despeckle_disc3", "gradient3", "mid_mixed", "hollow_max")


def drive(s, clear=True):
    TC.drive(s, RC.CAM, RC.LIGHT, clear)


def host(fb, case, edge="border", border=(0, 0, 0)):
    import tiny_renderer_amd as T
    return T.rank_host(fb, RC.params(case, edge, border))


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", RC.FRAMES, ids=["%dx%d" % s for s in RC.FRAMES])
def test_filtered_frame_equals_the_host_rule(small_synthetic, W, Hh):
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    fb = s.get_frame_buffer()
    assert fb.any()
    if (W, Hh) == (640, 480):
        flags = clean_flags(s)
        assert flags.any() and not flags.all(), "640 x 480 holds flagged and unflagged tiles"
    for name, case in ALL.items():
        for edge, border in RC.EDGES:
            same(s.get_ranked(RC.params(case, edge, border)), host(fb, case, edge, border), "%s %s %r" % (name, edge, border))
    same(s.get_ranked(RC.params(ALL["identity"])), fb, "one centre tap is a copy")
    same(s.get_frame_buffer(), fb, "the getter leaves the frame")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [640, 636], ids=["wide", "narrow"])
def test_device_pinned_and_getter_targets_between_guards(small_synthetic, W):
    """A device pointer at offset 0 and 1, a tensor, a tr_host_alloc block and the getter, each pre-filled with 0xAA between
    guard bytes: every byte inside is written, none outside; a pointer off by one byte gives the same image."""
    import torch
    import tiny_renderer_amd as T
    Hh = 480
    s = scene(W, Hh, small_synthetic, "specular")
    drive(s)
    fb = s.get_frame_buffer()
    L = T.load_library()
    for name in ("L_median", "15x15_rank224", "despeckle_disc3"):
        p = RC.params(ALL[name], "border", RC.PAPER)
        want = host(fb, ALL[name], "border", RC.PAPER)
        assert not (want == 0xAA).all()
        n = want.size
        dev = torch.full((n + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        for off in (0, 1):
            dev[:] = 0xAA
            torch.cuda.synchronize()
            s.rank(p, dev.data_ptr() + GUARD + off)
            assert s.sync() == 0
            raw = dev.cpu().numpy()
            same(raw[GUARD + off:GUARD + off + n].reshape(want.shape), want, "%s device + %d" % (name, off))
            assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
            dev[:] = 0xAA
            torch.cuda.synchronize()
            view = dev[GUARD + off:GUARD + off + n]
            assert s.rank(p, view) is view and s.sync() == 0
            raw = dev.cpu().numpy()
            same(raw[GUARD + off:GUARD + off + n].reshape(want.shape), want, "%s tensor + %d" % (name, off))
            assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
        block = L.tr_host_alloc(n + 2 * GUARD)
        assert block
        pinned = np.ctypeslib.as_array((C.c_uint8 * (n + 2 * GUARD)).from_address(block))
        pinned[:] = 0xAA
        assert L.tr_scene_rank(s._h, C.addressof(p), block) == 0 and s.sync() == 0
        same(pinned[:n].reshape(want.shape), want, name + " tr_host_alloc block")
        assert (pinned[n:] == 0xAA).all(), "bytes behind the picture changed"
        assert L.tr_scene_rank(s._h, C.addressof(p), block + 1) != 0, "an address inside a tr_host_alloc block is no `out`"
        L.tr_host_free(block)
        mine = s.pinned_frame()
        mine[...] = 0xAA
        assert s.rank(p, mine) is mine and s.sync() == 0
        same(mine, want, name + " pinned_frame")
        guarded = np.full(n + 2 * GUARD, 0xAA, np.uint8)
        assert L.tr_scene_get_ranked(s._h, C.addressof(p), guarded[GUARD:].ctypes.data) == 0
        same(guarded[GUARD:GUARD + n].reshape(want.shape), want, name + " getter")
        assert (guarded[:GUARD] == 0xAA).all() and (guarded[GUARD + n:] == 0xAA).all()
    same(s.get_frame_buffer(), fb, "out of place leaves the frame")
    s.close()


DENSE = [(W, Hh, kind) for W, Hh in DC.SIZES_HALO for kind in DC.BACKDROPS]


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh,kind", DENSE, ids=["%dx%d-%s" % r for r in DENSE])
def test_dense_frames_in_a_callers_buffer(small_synthetic, W, Hh, kind):
    """Rendered frames are smooth and mostly black, and a median of them is mostly its input: noise, white and the planted
    picture in a caller's guarded buffer, drawn into without a clear.  On noise the median differs from its input."""
    s, buf, f = TD.dense_scene(small_synthetic, W, Hh, kind)
    for name in SUBSET + ("3x3_rank0", "3x3_rank8", "line30_median", "clamp_extremes"):
        for edge, border in RC.EDGES:
            want = host(f["fb"], ALL[name], edge, border)
            if kind == "noise" and name in ("3x3_rank4", "15x15_rank112", "L_median"):
                assert not np.array_equal(want, f["fb"]), name + ": the median of noise is the noise"
            same(s.get_ranked(RC.params(ALL[name], edge, border)), want, "%s %s %r" % (name, edge, border))
    TD.in_buffer(buf, f["fb"])
    s.close()


@pytest.mark.gpu
def test_stale_memory_behind_raised_flags_and_the_cleared_scene(small_synthetic):
    """A frame that covers the screen, then a clear and the small model: tiles lit in the first frame and flagged clean in
    the second hold the first frame's bytes in memory and must read as zeros.  Then the cleared scene's short-circuits on the
    k_rank launch count."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = 640, 480
    s = T.Scene(W, Hh, mesh, texs, "phong")
    s.set_instances(np.array([[0.0, 0.0, 0.0, 3.0]], np.float32))
    TR.frame(s, 0.0, 0.0)
    one = s.get_frame_buffer()
    flags_one, t = TR.clean_flags(s)
    lit_one = TR.lit_tiles(one, t)
    assert lit_one.mean() > 0.9
    s.set_instances(None)
    TR.frame(s)
    two = s.get_frame_buffer()
    flags_two, _ = TR.clean_flags(s)
    assert (lit_one & ~flags_one & flags_two).any(), "no tile lit in frame one is flagged clean in frame two"
    for name in SUBSET + ("3x3_rank8", "15x15_rank224"):
        for edge, border in RC.EDGES:
            same(s.get_ranked(RC.params(ALL[name], edge, border)), host(two, ALL[name], edge, border), "%s %s %r" % (name, edge, border))
    median, dilate = ALL["15x15_rank112"], ALL["3x3_rank8"]
    s.profile_enable(True)
    s.clear()
    dev = device_buffer(W * Hh * 3)
    s.rank(RC.params(median, "clamp", RC.PAPER), dev.data_ptr())
    assert s.sync() == 0 and not dev.cpu().numpy().any(), "a cleared scene ranks to zeros"
    s.clear()
    assert not s.get_ranked(RC.params(median)).any() and not s.get_ranked(RC.params(ALL["gradient3"], "clamp")).any()
    assert s.rank(RC.params(dilate)) is None and s.sync() == 0
    assert "k_rank" not in s.profile_read(), "a cleared scene launches nothing where no border colour comes in"
    black = np.zeros((Hh, W, 3), np.uint8)
    s.clear()
    want = host(black, dilate, "border", RC.PAPER)
    assert want.any() and not want.all()
    same(s.get_ranked(RC.params(dilate, "border", RC.PAPER)), want, "a cleared scene under another border")
    assert s.profile_read()["k_rank"]["launches"] == 1
    assert not s.get_frame_buffer().any()
    s.clear()
    s.rank(RC.params(dilate, "border", RC.PAPER))
    same(s.get_frame_buffer(), want, "a cleared scene in place under another border")
    flags = clean_flags(s)
    assert flags.any() and not (flags & TR.lit_tiles(want, s.band_tiles())).any(), "the frame of paper is flagged clean, or no inner tile is"
    assert s.profile_read()["k_rank"]["launches"] == 2
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(640, 480), (134, 21)], ids=["whole_tile_rows", "partial_tile_row"])
def test_in_place_the_frame_and_its_flags_follow(small_synthetic, W, Hh):
    """The frame afterwards is the out-of-place result; resize, resolve and the sparse read-back see it; z stays; applied
    twice; erode then dilate is the host's open; a later clear and render is the caller's."""
    import tiny_renderer_amd as T
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    before = snap(s)
    fb = before["fb"]
    for name, edge, border in (("15x15_rank112", "border", (0, 0, 0)), ("L_median", "border", RC.PAPER), ("gradient3", "clamp", (0, 0, 0)), ("3x3_rank8", "clamp", (0, 0, 0))):
        case = ALL[name]
        want = host(fb, case, edge, border)
        assert not np.array_equal(want, fb)
        drive(s)
        assert s.rank(RC.params(case, edge, border)) is None
        flags = clean_flags(s)
        lit = TR.lit_tiles(want, s.band_tiles())
        assert not (flags & lit).any(), "a tile that holds colour is flagged clean"
        if (W, Hh) == (640, 480) and border == (0, 0, 0):
            assert flags.any(), "no tile is flagged clean"
        same(s.get_frame_buffer(), want, name + ": the frame afterwards")
        pinned = s.pinned_frame()
        pinned[...] = 0xAA
        s.get_frame_buffer_async(pinned)
        assert s.sync() == 0
        same(pinned, want, name + ": the sparse read-back")
        same(s.resize(W // 2 + 1, Hh // 2 + 1), T.resize_host(want, W // 2 + 1, Hh // 2 + 1), name + ": resize afterwards")
        if W % 2 == 0 and Hh % 2 == 0:
            same(s.resolve(2), TR.box(want, 2), name + ": resolve afterwards")
        assert np.array_equal(TC.bits(s.read_z_f32()), TC.bits(before["z"])), "z changed"
        s.rank(RC.params(case, edge, border))
        same(s.get_frame_buffer(), host(want, case, edge, border), name + ": twice")
    drive(s)
    disc = T.footprint_disc(2)
    erode, dilate = T.rank_params(disc, "min", edge="clamp"), T.rank_params(disc, "max", edge="clamp")
    s.rank(erode), s.rank(dilate)
    opened = T.rank_host(T.rank_host(fb, erode), dilate)
    assert not np.array_equal(opened, fb) and opened.any()
    same(s.get_frame_buffer(), opened, "erode then dilate is the host's open")
    drive(s)
    TC.same(snap(s), before)
    s.close()


@pytest.mark.gpu
def test_a_rank_between_two_renders_is_ordered_on_the_stream(small_synthetic):
    import torch
    W, Hh = 300, 200
    s = scene(W, Hh, small_synthetic, "phong", frames_per_launch=4)
    drive(s)
    fb = s.get_frame_buffer()
    a = torch.full((W * Hh * 3,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    TR.frame(s, RC.CAM, RC.LIGHT)
    s.rank(RC.params(ALL["15x15_rank112"], "clamp"), a)
    TR.frame(s, 1.1, 0.2)
    assert s.sync() == 0
    two = s.get_frame_buffer()
    assert not np.array_equal(two, fb)
    same(a.cpu().numpy().reshape(Hh, W, 3), host(fb, ALL["15x15_rank112"], "clamp"), "the first frame, filtered before the second was rendered")
    s.close()


@pytest.mark.gpu
def test_no_depth_pass_is_provoked_and_the_profile_counts_the_launches(small_synthetic):
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong")
    s.profile_enable(True)
    drive(s)
    assert s.sync() == 0
    tiles = dict(s.profile_read())
    p = RC.params(ALL["L_median"])
    s.get_ranked(p)
    s.rank(RC.params(ALL["3x3_rank0"], "clamp"), device_buffer(W * Hh * 3).data_ptr())
    s.rank(p)
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_rank", {}).get("launches") == 3 and prof["k_rank"]["total_ms"] > 0.0, prof
    for k in ("k_tile", "k_tile_depth"):
        assert prof.get(k, {}).get("launches", 0) == tiles.get(k, {}).get("launches", 0), (k, tiles, prof)
    assert prof["k_tile"]["launches"] >= 1
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", PIPELINES)
def test_every_pipeline(small_synthetic, pipe):
    W, Hh = 640, 480
    s = scene(W, Hh, small_synthetic, pipe)
    drive(s)
    fb = s.get_frame_buffer()
    drive(s)
    same(s.get_ranked(RC.params(ALL["despeckle_disc3"], "border", RC.PAPER)), host(fb, ALL["despeckle_disc3"], "border", RC.PAPER), pipe)
    s.close()


@pytest.mark.gpu
def test_refusals_leave_the_scene_alone(small_synthetic):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import _lib
    L = T.load_library()
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong", tap=True)
    band = scene(W, Hh, small_synthetic, "phong", band_rows=(16, 32))
    drive(s), drive(band)
    before, flags = snap(s), clean_flags(s)
    before_band, flags_band = snap(band), clean_flags(band)
    p = RC.params(ALL["3x3_rank4"])
    q = C.addressof(p)
    host_out = np.full((Hh, W, 3), 0xAA, np.uint8)
    dev = device_buffer(W * Hh * 3)
    text = lambda: L.tr_last_error().decode()
    calls = (("tr_scene_rank", lambda sc, pp: L.tr_scene_rank(sc._h, pp, dev.data_ptr())),
             ("tr_scene_get_ranked", lambda sc, pp: L.tr_scene_get_ranked(sc._h, pp, host_out.ctypes.data)))

    def wrong(**kw):
        w = RC.params(ALL["3x3_rank4"])
        for k, v in kw.items():
            if k.startswith("row"):
                w.rows[int(k[3:])] = v
            else:
                setattr(w, k, v)
        return w

    for who, call in calls:
        assert call(s, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        for kw, why in ((dict(struct_size=60), ": struct_size is not sizeof(tr_rank_params)"), (dict(kw=2), ": kw and kh must be odd and 1..15"),
                        (dict(kh=17), ": kw and kh must be odd and 1..15"), (dict(row0=0xF), ": footprint bits outside the kw x kh box"),
                        (dict(row3=1), ": footprint bits outside the kw x kh box"), (dict(row0=0, row1=0, row2=0), ": the footprint is empty"),
                        (dict(op=4), ": op must be TR_RANK_VALUE, TR_RANK_RANGE, TR_RANK_MID or TR_RANK_CLAMP_CENTRE"),
                        (dict(edge=2), ": edge must be TR_RANK_BORDER or TR_RANK_CLAMP"), (dict(pad=1), ": pad and pad2 must be 0"), (dict(pad2=1), ": pad and pad2 must be 0"),
                        (dict(rank=9), ": rank and rank2 must be below the number of taps"), (dict(op=2, rank2=9), ": rank and rank2 must be below the number of taps"),
                        (dict(op=1, rank=5, rank2=4), ": rank must not exceed rank2"), (dict(rank2=1), ": rank2 must be 0 under TR_RANK_VALUE")):
            assert call(s, C.addressof(wrong(**kw))) == _lib.TR_E_INVALID and text() == who + why
        # which refusal wins: the parameters before the band, the band before the target
        assert call(band, C.addressof(wrong(rank=9))) == _lib.TR_E_INVALID and text() == who + ": rank and rank2 must be below the number of taps"
        assert call(band, q) == _lib.TR_E_INVALID
        assert text() == who + ": a band scene (tr_options.band_row0/1) cannot be ranked: its border taps lie in another rank's rows"
    assert L.tr_scene_rank(None, q, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_rank: null scene"
    assert L.tr_scene_get_ranked(None, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_ranked: null scene"
    assert L.tr_scene_get_ranked(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_ranked: null argument"
    assert L.tr_scene_rank(band._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text().startswith("tr_scene_rank: a band scene")
    with pytest.raises(T.TinyRendererError):
        band.get_ranked(p)
    assert L.tr_scene_rank(s._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_rank: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_ranked takes any host memory)"
    small = L.tr_host_alloc(W * Hh * 3 - 1)
    assert small
    assert L.tr_scene_rank(s._h, q, small) == _lib.TR_E_INVALID and text() == "tr_scene_rank: the host buffer is smaller than the frame"
    L.tr_host_free(small)
    t = s.band_tiles()
    assert L.tr_scene_rank(s._h, q, int(t.frame_buffer_device) + 3) == _lib.TR_E_INVALID
    assert text() == "tr_scene_rank: `out` overlaps a frame buffer of the scene (out == NULL ranks in place)"
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    for q_, f_, fl_, rows in ((s, before, flags, None), (band, before_band, flags_band, (16, 32))):
        assert q_.sync() == 0
        assert np.array_equal(clean_flags(q_), fl_)
        TC.same(snap(q_), f_, rows)
    s.close(), band.close()


@pytest.mark.gpu
def test_cli_options_write_the_filtered_picture(african_head, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    common = ["-p", H.asset_dir("african_head"), "-s", "phong", "--width", "640", "--height", "480", "--camera-angle", "0.3", "--light-angle", "0.7"]
    names = ("full", "median", "erode", "dilate", "despeckle", "chain", "blurred")
    full, median, erode, dilate, despeckle, chain, blurred = (str(tmp_path / (n + ".ppm")) for n in names)
    assert cli.main(common + ["--out", full]) == 0
    assert cli.main(common + ["--median", "2", "--out", median]) == 0
    assert cli.main(common + ["--erode", "1", "--rank-shape", "cross", "--out", erode]) == 0
    assert cli.main(common + ["--dilate", "3", "--rank-shape", "disc", "--out", dilate]) == 0
    assert cli.main(common + ["--despeckle", "1", "--out", despeckle]) == 0
    assert cli.main(common + ["--despeckle", "1", "--median", "1", "--dilate", "2", "--erode", "2", "--rank-shape", "disc", "--out", chain]) == 0
    assert cli.main(common + ["--blur", "2.5", "--median", "1", "--out", blurred]) == 0
    hd = b"P6\n640 480\n255\n"
    a, b, c, d, e, f, g = (np.frombuffer(open(p, "rb").read()[len(hd):], np.uint8).reshape(480, 640, 3) for p in (full, median, erode, dilate, despeckle, chain, blurred))
    assert a.any()
    rank = lambda img, fp, *r, **kw: T.rank_host(img, T.rank_params(fp, *r, edge="clamp", **kw))
    same(b, rank(a, T.footprint_rect(5, 5), "median"), "--median")
    same(c, rank(a, T.footprint_cross(1), "min"), "--erode")
    same(d, rank(a, T.footprint_disc(3), "max"), "--dilate")
    same(e, rank(a, T.footprint_rect(3, 3), 1, 7, op="clamp_centre"), "--despeckle")
    d2, d1 = T.footprint_disc(2), T.footprint_disc(1)
    step = rank(rank(a, d2, "min"), d2, "max")
    same(f, rank(rank(step, d1, "median"), d1, 1, 7, op="clamp_centre"), "erode, dilate, median, despeckle in this order")
    k, shift = T.kernel_gaussian(2.5)
    same(g, rank(T.convolve_host(a, T.convolve_params(k, shift=shift, edge="clamp")), T.footprint_rect(3, 3), "median"), "--blur before --median")
    assert not np.array_equal(b, a) and not np.array_equal(c, a)
    for bad in (["--median", "2", "--view", "z"], ["--median", "0"], ["--erode", "8"], ["--median", "x"], ["--median", "1", "--median", "2"],
                ["--rank-shape", "disc"], ["--dilate", "2", "--seconds", "1"], ["--despeckle", "1", "--rank-shape", "line"]):
        with pytest.raises(SystemExit):
            cli.main(common + bad)
