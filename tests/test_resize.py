"""Resize on the device: tr_scene_resize / tr_scene_get_resized (k_resize) equal tr_resize_host in every byte.

Every comparison is np.array_equal against resize_host of the frame the scene itself returns; tests/test_resize_host.py
pins resize_host against numpy and the tables against the rule in Python integers.  The sizes are tests/resize_cases.py's:
four sources (a width that is no multiple of 4 with one partial tile row; flagged and unflagged tiles; two odd ones) and
per source the outputs at the ends of the allowed ratios, one past a multiple of every compiled tile, and across them."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import resize_cases as RC
from tests import test_composite as TC
from tests import test_outline as TO
from tests import test_resolve as TR

bits, scene, snap, clean_flags, tiles_any = TC.bits, TC.scene, TC.snap, TC.clean_flags, TC.tiles_any
device_buffer, box = TO.device_buffer, TO.box
PIPELINES = TR.PIPELINES
GUARD = 64


def drive(s, cam=RC.CAM, light=RC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def host(fb, w, h, filt="area"):
    import tiny_renderer_amd as T
    return T.resize_host(fb, w, h, filt)


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("filt", RC.FILTERS)
@pytest.mark.parametrize("W,Hh", RC.SOURCES, ids=["%dx%d" % s for s in RC.SOURCES])
def test_resized_frame_equals_the_host_rule(small_synthetic, W, Hh, filt):
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    fb = s.get_frame_buffer()
    assert fb.any() and not fb.all(-1).all()
    if (W, Hh) == (640, 480):
        flags = clean_flags(s)
        assert flags.any() and not flags.all(), "640 x 480 holds flagged and unflagged tiles"
    for w, h in RC.outputs(W, Hh):
        drive(s)
        same(s.resize(w, h, filt), host(fb, w, h, filt), "%dx%d %s" % (w, h, filt))
        if filt == "area" and (w, h) == (W, Hh):
            same(s.resize(w, h, filt), fb, "the same size is a copy")
        for f in (2, 4):
            if filt == "area" and W % f == 0 and Hh % f == 0 and (w, h) == (W // f, Hh // f):
                same(s.resize(w, h, filt), s.resolve(f), "area by %d is k_resolve's box filter" % f)
    if filt == "area" and W % 8 == 0 and Hh % 8 == 0:
        same(s.resize(W // 8, Hh // 8), s.resolve(8), "area by 8 is k_resolve's box filter")
    s.close()


@pytest.mark.gpu
def test_one_pixel_from_the_smallest_scene(small_synthetic):
    """8 x 8 -> 1 x 1 (tr_scene_create accepts the size), and one row of tiles out of it."""
    s = scene(8, 8, small_synthetic, "phong")
    drive(s)
    fb = s.get_frame_buffer()
    assert fb.any()
    for filt in RC.FILTERS:
        same(s.resize(1, 1, filt), host(fb, 1, 1, filt), "8x8 -> 1x1 " + filt)
        same(s.resize(64, 3, filt), host(fb, 64, 3, filt), "8x8 -> 64x3 " + filt)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", PIPELINES)
def test_every_pipeline(small_synthetic, pipe):
    s = scene(640, 480, small_synthetic, pipe)
    drive(s)
    fb = s.get_frame_buffer()
    drive(s)
    same(s.resize(427, 320), host(fb, 427, 320), pipe)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filt", RC.FILTERS)
@pytest.mark.parametrize("w,h", [(428, 320), (427, 321)], ids=["wide", "narrow"])
def test_device_pinned_and_getter_targets_between_guards(small_synthetic, w, h, filt):
    """A torch tensor, a tr_host_alloc block and the getter, each pre-filled with 0xAA between guard bytes: every byte
    inside is written, none outside.  A device pointer off by one byte takes the narrow path and gives the same image."""
    import torch
    import tiny_renderer_amd as T
    s = scene(640, 480, small_synthetic, "specular")
    drive(s)
    want = host(s.get_frame_buffer(), w, h, filt)
    assert (want == 0).all(-1).any() and want.any() and not (want == 0xAA).all()
    n = want.size
    dev = torch.full((n + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for off in (0, 1):
        dev[:] = 0xAA
        torch.cuda.synchronize()
        drive(s)
        s.resize_into(dev.data_ptr() + GUARD + off, w, h, filt)
        assert s.sync() == 0
        raw = dev.cpu().numpy()
        same(raw[GUARD + off:GUARD + off + n].reshape(want.shape), want, "device + %d" % off)
        assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
    whole = torch.full((h, w, 3), 0xAA, dtype=torch.uint8, device="cuda")
    assert s.resize_into(whole, w, h, filt) is whole
    assert s.sync() == 0
    same(whole.cpu().numpy(), want, "tensor")
    L = T.load_library()
    block = L.tr_host_alloc(n + 2 * GUARD)
    assert block
    pinned = np.ctypeslib.as_array((C.c_uint8 * (n + 2 * GUARD)).from_address(block))
    pinned[:] = 0xAA
    p = T.resize_params(640, 480, w, h, filt)
    assert L.tr_scene_resize(s._h, C.addressof(p), block) == 0 and s.sync() == 0
    same(pinned[:n].reshape(want.shape), want, "tr_host_alloc block")
    assert (pinned[n:] == 0xAA).all(), "bytes behind the picture changed"
    L.tr_host_free(block)
    mine = s.pinned_resized(w, h)
    mine[...] = 0xAA
    assert s.resize_into(mine, w, h, filt) is mine and s.sync() == 0
    same(mine, want, "pinned_resized")
    guarded = np.full(n + 2 * GUARD, 0xAA, np.uint8)
    assert L.tr_scene_get_resized(s._h, C.addressof(p), guarded[GUARD:].ctypes.data) == 0
    same(guarded[GUARD:GUARD + n].reshape(want.shape), want, "getter")
    assert (guarded[:GUARD] == 0xAA).all() and (guarded[GUARD + n:] == 0xAA).all()
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("filt", RC.FILTERS)
def test_tiles_flagged_clean_contribute_zeros_whatever_came_before(small_synthetic, filt):
    """A frame that covers the screen, then a clear and the small model: tiles lit in the first frame and flagged clean in
    the second contribute the second frame's zeros.  Then the cleared scene's short-circuit."""
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
    for w, h in ((80, 60), (427, 320), (640, 480), (700, 500), (1280, 960)):
        same(s.resize(w, h, filt), host(two, w, h, filt), "%dx%d" % (w, h))
    s.profile_enable(True)
    s.clear()
    dev = device_buffer(91 * 77 * 3)
    s.resize_into(dev.data_ptr(), 91, 77, filt)
    assert s.sync() == 0 and not dev.cpu().numpy().any(), "a cleared scene resizes to zeros"
    s.clear()
    assert not s.resize(91, 77, filt).any()
    assert "k_resize" not in s.profile_read(), "a cleared scene launches nothing"
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["noise", "white"])
def test_a_dense_frame_in_a_callers_buffer(small_synthetic, kind):
    """tests/dense_cases.py's frames: a caller's buffer of noise (or white) drawn into without a clear.  No flag may be
    trusted there; white stays white where nothing is drawn."""
    from tests import test_dense_frames as TD
    W, Hh = 256, 48
    s, buf, f = TD.dense_scene(small_synthetic, W, Hh, kind)
    for filt in RC.FILTERS:
        for w, h in ((32, 6), (33, 7), (128, 24), (256, 48), (257, 47), (300, 100)):
            same(s.resize(w, h, filt), host(f["fb"], w, h, filt), "%s %dx%d %s" % (kind, w, h, filt))
    TD.in_buffer(buf, f["fb"])
    s.close()


@pytest.mark.gpu
def test_ordering_kept_frames_and_the_table_cache(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = 300, 200
    s = T.Scene(W, Hh, mesh, texs, "phong", frames_per_launch=4)
    # held-back frames are submitted, and a later render is ordered behind the resize
    a, b = torch.full((97 * 65 * 3,), 0xAA, dtype=torch.uint8, device="cuda"), torch.full((97 * 65 * 3,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    TR.frame(s, 0.3, 0.7)
    s.resize_into(a.data_ptr(), 97, 65)
    TR.frame(s, 1.1, 0.2)
    s.resize_into(b.data_ptr(), 97, 65, "bilinear")
    assert s.sync() == 0
    two = s.get_frame_buffer()
    TR.frame(s, 0.3, 0.7)
    one = s.get_frame_buffer()
    assert not np.array_equal(one, two)
    same(a.cpu().numpy().reshape(65, 97, 3), host(one, 97, 65), "the first frame, resized before the second was rendered")
    same(b.cpu().numpy().reshape(65, 97, 3), host(two, 97, 65, "bilinear"), "the second frame")
    # kept frames of a group, one by one
    params = TR._params(3)
    s.render_frames(params)
    frames = []
    for back in range(3):
        s.select_frame(back)
        frames.append(s.get_frame_buffer())
    assert not np.array_equal(frames[0], frames[1])
    s.render_frames(params)
    for back in range(3):
        s.select_frame(back)
        same(s.resize(211, 97), host(frames[back], 211, 97), "kept frame %d" % back)
    # two sizes (and filters) alternate: the tables follow
    s.select_frame(0)
    for i in range(5):
        same(s.resize(65, 25, "bilinear"), host(frames[0], 65, 25, "bilinear"), "round %d, small" % i)
        same(s.resize(129, 209), host(frames[0], 129, 209), "round %d, large" % i)
        same(s.resize(129, 209, "bilinear"), host(frames[0], 129, 209, "bilinear"), "round %d, the other filter" % i)
    # ... and without a wait between the calls
    outs = [torch.full((65 * 25 * 3,), 0xAA, dtype=torch.uint8, device="cuda") for _ in range(3)]
    bigs = [torch.full((129 * 209 * 3,), 0xAA, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    for o, g in zip(outs, bigs):
        s.resize_into(o, 65, 25)
        s.resize_into(g, 129, 209)
    assert s.sync() == 0
    for o, g in zip(outs, bigs):
        same(o.cpu().numpy().reshape(25, 65, 3), host(frames[0], 65, 25), "queued, small")
        same(g.cpu().numpy().reshape(209, 129, 3), host(frames[0], 129, 209), "queued, large")
    s.close()


@pytest.mark.gpu
def test_after_grade_and_antialias_in_place(small_synthetic):
    import tiny_renderer_amd as T
    from tests import test_grade as TG
    W, Hh = 300, 200
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    fb = s.get_frame_buffer()
    lut = TG.random_lut(17, 5)
    graded = T.grade_host(fb, lut)
    smooth = T.aa_host(fb, T.aa_params())
    assert not np.array_equal(graded, fb) and not np.array_equal(smooth, fb)
    drive(s)
    s.set_lut(lut), s.grade()
    same(s.resize(211, 97), host(graded, 211, 97), "after grade in place")
    drive(s)
    s.antialias(T.aa_params())
    same(s.resize(211, 97, "bilinear"), host(smooth, 211, 97, "bilinear"), "after antialias in place")
    s.close()


@pytest.mark.gpu
def test_no_depth_pass_is_provoked_and_the_profile_counts_the_launches(small_synthetic):
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong")
    s.profile_enable(True)
    drive(s)
    assert s.sync() == 0
    tiles = dict(s.profile_read())
    s.resize(100, 30)
    s.resize_into(device_buffer(64 * 48 * 3).data_ptr(), 64, 48, "bilinear")
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_resize", {}).get("launches") == 2 and prof["k_resize"]["total_ms"] > 0.0, prof
    for k in ("k_tile", "k_tile_depth"):
        assert prof.get(k, {}).get("launches", 0) == tiles.get(k, {}).get("launches", 0), (k, tiles, prof)
    assert prof["k_tile"]["launches"] >= 1
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
    p = T.resize_params(W, Hh, 100, 30)
    q = C.addressof(p)
    host_out = np.full((30, 100, 3), 0xAA, np.uint8)
    dev = device_buffer(100 * 30 * 3)
    text = lambda: L.tr_last_error().decode()
    band_text = ": a band scene (tr_options.band_row0/1) cannot be resized: its border taps lie in another rank's rows"
    assert L.tr_scene_resize(band._h, q, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_resize" + band_text
    assert L.tr_scene_get_resized(band._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_resized" + band_text
    with pytest.raises(T.TinyRendererError):
        band.resize(100, 30)
    assert L.tr_scene_resize(s._h, q, None) == _lib.TR_E_INVALID
    assert text() == "tr_scene_resize: out == NULL (the output is no frame of the scene: there is no in-place form)"
    with pytest.raises(ValueError):
        s.resize_into(None, 100, 30)
    assert L.tr_scene_resize(s._h, None, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_resize: null argument"
    assert L.tr_scene_get_resized(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_resized: null argument"
    shrinks = ": a side shrinks by more than 8 (width and height must be at least an eighth of the source's, rounded up)"
    for fields, why in (((31, 6, 0, 0), shrinks), ((32, 5, 0, 0), shrinks), ((0, 6, 0, 0), ": width and height must be 1..8192"),
                        ((8193, 6, 0, 0), ": width and height must be 1..8192"), ((32, 6, 2, 0), ": filter must be TR_RESIZE_AREA or TR_RESIZE_BILINEAR"),
                        ((32, 6, 0, 4), ": flags must be 0")):
        bad = T.ResizeParams(*fields)
        assert L.tr_scene_resize(s._h, C.addressof(bad), dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_resize" + why
        assert L.tr_scene_get_resized(s._h, C.addressof(bad), host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_resized" + why
    assert L.tr_scene_resize(s._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_resize: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_resized takes any host memory)"
    small = L.tr_host_alloc(100 * 30 * 3 - 1)
    assert small
    assert L.tr_scene_resize(s._h, q, small) == _lib.TR_E_INVALID and text() == "tr_scene_resize: the host buffer is smaller than the resized frame"
    L.tr_host_free(small)
    with pytest.raises(ValueError) as e:
        s.resize(31, 6)
    assert str(e.value) == "tr_scene_get_resized" + shrinks
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    for q_, f_, fl_, rows in ((s, before, flags, None), (band, before_band, flags_band, (16, 32))):
        assert q_.sync() == 0
        assert np.array_equal(clean_flags(q_), fl_)
        TC.same(snap(q_), f_, rows)
    s.close(), band.close()


@pytest.mark.gpu
def test_cli_out_size_writes_the_resized_picture(african_head, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    common = ["-p", H.asset_dir("african_head"), "-s", "phong", "--width", "640", "--height", "480", "--camera-angle", "0.3", "--light-angle", "0.7"]
    full, area, bil = (str(tmp_path / n) for n in ("full.ppm", "area.ppm", "bilinear.ppm"))
    assert cli.main(common + ["--out", full]) == 0
    assert cli.main(common + ["--out-size", "427x320", "--out", area]) == 0
    assert cli.main(common + ["--out-size", "427x320", "--resize-filter", "bilinear", "--out", bil]) == 0
    a = np.frombuffer(open(full, "rb").read()[len(b"P6\n640 480\n255\n"):], np.uint8).reshape(480, 640, 3)
    hd = b"P6\n427 320\n255\n"
    assert open(area, "rb").read().startswith(hd)
    b, c = (np.frombuffer(open(p, "rb").read()[len(hd):], np.uint8).reshape(320, 427, 3) for p in (area, bil))
    assert a.any()
    same(b, T.resize_host(a, 427, 320, "area"), "--out-size")
    same(c, T.resize_host(a, 427, 320, "bilinear"), "--resize-filter bilinear")
    assert not np.array_equal(b, c)
    for bad in (["--out-size", "427x320", "--ssaa", "2"], ["--out-size", "427x320", "--view", "z"], ["--out-size", "10x10"], ["--out-size", "427"]):
        with pytest.raises(SystemExit):
            cli.main(common + bad)
