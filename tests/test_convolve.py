"""Convolve on the device: tr_scene_convolve / tr_scene_get_convolved (k_convolve) equal tr_convolve_host in every byte.

Every comparison is np.array_equal against convolve_host of the frame the scene itself returns; tests/test_convolve_host.py
pins convolve_host against the rule in numpy int64.  Kernels, edges and frame sizes are tests/convolve_cases.py's."""
import ctypes as C

import numpy as np
import pytest

from tests import convolve_cases as CC
from tests import dense_cases as DC
from tests import helpers as H
from tests import test_composite as TC
from tests import test_dense_frames as TD
from tests import test_outline as TO
from tests import test_resolve as TR

scene, snap, clean_flags = TC.scene, TC.snap, TC.clean_flags
device_buffer = TO.device_buffer
PIPELINES = TR.PIPELINES
GUARD = 64
ALL = CC.everything()
SUBSET = ("9x9_alternating", "emboss", "gaussian31", "extreme", "unsharp", "3x5")


def drive(s, clear=True):
    TC.drive(s, CC.CAM, CC.LIGHT, clear)


def host(fb, case, edge="border", border=(0, 0, 0)):
    import tiny_renderer_amd as T
    return T.convolve_host(fb, CC.params(case, edge, border))


def same(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", CC.FRAMES, ids=["%dx%d" % s for s in CC.FRAMES])
def test_filtered_frame_equals_the_host_rule(small_synthetic, W, Hh):
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    fb = s.get_frame_buffer()
    assert fb.any()
    if (W, Hh) == (640, 480):
        flags = clean_flags(s)
        assert flags.any() and not flags.all(), "640 x 480 holds flagged and unflagged tiles"
    for name, case in ALL.items():
        for edge, border in CC.EDGES:
            same(s.get_convolved(CC.params(case, edge, border)), host(fb, case, edge, border), "%s %s %r" % (name, edge, border))
    same(s.get_convolved(CC.params(ALL["identity"])), fb, "1 x 1 is a copy")
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
    for name in ("emboss", "gaussian31", "unsharp"):
        p = CC.params(ALL[name], "border", CC.PAPER)
        want = host(fb, ALL[name], "border", CC.PAPER)
        assert not (want == 0xAA).all()
        n = want.size
        dev = torch.full((n + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
        for off in (0, 1):
            dev[:] = 0xAA
            torch.cuda.synchronize()
            s.convolve(p, dev.data_ptr() + GUARD + off)
            assert s.sync() == 0
            raw = dev.cpu().numpy()
            same(raw[GUARD + off:GUARD + off + n].reshape(want.shape), want, "%s device + %d" % (name, off))
            assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
            # the same through a tensor: a view of the guarded buffer at the same offset
            dev[:] = 0xAA
            torch.cuda.synchronize()
            view = dev[GUARD + off:GUARD + off + n]
            assert s.convolve(p, view) is view and s.sync() == 0
            raw = dev.cpu().numpy()
            same(raw[GUARD + off:GUARD + off + n].reshape(want.shape), want, "%s tensor + %d" % (name, off))
            assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
        # a tr_host_alloc block is known to the library by its first byte (classify_out), as for every stage: the picture
        # starts there, offset 0, with guard bytes behind it
        block = L.tr_host_alloc(n + 2 * GUARD)
        assert block
        pinned = np.ctypeslib.as_array((C.c_uint8 * (n + 2 * GUARD)).from_address(block))
        pinned[:] = 0xAA
        assert L.tr_scene_convolve(s._h, C.addressof(p), block) == 0 and s.sync() == 0
        same(pinned[:n].reshape(want.shape), want, name + " tr_host_alloc block")
        assert (pinned[n:] == 0xAA).all(), "bytes behind the picture changed"
        assert L.tr_scene_convolve(s._h, C.addressof(p), block + 1) != 0, "an address inside a tr_host_alloc block is no `out`"
        L.tr_host_free(block)
        mine = s.pinned_frame()
        mine[...] = 0xAA
        assert s.convolve(p, mine) is mine and s.sync() == 0
        same(mine, want, name + " pinned_frame")
        guarded = np.full(n + 2 * GUARD, 0xAA, np.uint8)
        assert L.tr_scene_get_convolved(s._h, C.addressof(p), guarded[GUARD:].ctypes.data) == 0
        same(guarded[GUARD:GUARD + n].reshape(want.shape), want, name + " getter")
        assert (guarded[:GUARD] == 0xAA).all() and (guarded[GUARD + n:] == 0xAA).all()
    same(s.get_frame_buffer(), fb, "out of place leaves the frame")
    s.close()


DENSE = [(W, Hh, kind) for W, Hh in DC.SIZES_HALO for kind in DC.BACKDROPS]


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh,kind", DENSE, ids=["%dx%d-%s" % r for r in DENSE])
def test_dense_frames_in_a_callers_buffer(small_synthetic, W, Hh, kind):
    """Rendered frames are smooth and mostly black and would hide a sign error or an overflow: noise, white and the planted
    picture in a caller's guarded buffer, drawn into without a clear, through the kernels at the bounds (both 24-bit forms
    at their limit, the 32-bit form, A = 2^22 without cancellation), the Gaussian, the emboss and the unsharp mask."""
    s, buf, f = TD.dense_scene(small_synthetic, W, Hh, kind)
    for name in CC.EXTREME + ("gaussian31", "emboss", "unsharp"):
        for edge, border in CC.EDGES:
            same(s.get_convolved(CC.params(ALL[name], edge, border)), host(f["fb"], ALL[name], edge, border), "%s %s %r" % (name, edge, border))
    TD.in_buffer(buf, f["fb"])
    s.close()


@pytest.mark.gpu
def test_stale_memory_behind_raised_flags_and_the_cleared_scene(small_synthetic):
    """A frame that covers the screen, then a clear and the small model: tiles lit in the first frame and flagged clean in
    the second hold the first frame's bytes in memory and must read as zeros.  Then the cleared scene's short-circuits on the
    k_convolve launch count."""
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
    for name in SUBSET + ("box3", "tent15"):
        for edge, border in CC.EDGES:
            same(s.get_convolved(CC.params(ALL[name], edge, border)), host(two, ALL[name], edge, border), "%s %s %r" % (name, edge, border))
    blur, emboss = ALL["gaussian31"], ALL["emboss"]
    s.profile_enable(True)
    s.clear()
    dev = device_buffer(W * Hh * 3)
    s.convolve(CC.params(blur, "clamp", CC.PAPER), dev.data_ptr())
    assert s.sync() == 0 and not dev.cpu().numpy().any(), "a cleared scene blurs to zeros"
    s.clear()
    assert not s.get_convolved(CC.params(blur)).any() and not s.get_convolved(CC.params(ALL["unsharp"], "clamp")).any()
    assert s.convolve(CC.params(blur)) is None and s.sync() == 0
    assert "k_convolve" not in s.profile_read(), "a cleared scene launches nothing where the rule gives black"
    black = np.zeros((Hh, W, 3), np.uint8)
    s.clear()
    same(s.get_convolved(CC.params(blur, "border", CC.PAPER)), host(black, blur, "border", CC.PAPER), "a cleared scene under another border")
    assert s.profile_read()["k_convolve"]["launches"] == 1
    s.clear()
    want = host(black, emboss, "clamp")
    assert (want == 128).all()
    same(s.get_convolved(CC.params(emboss, "clamp")), want, "a cleared scene under a bias")
    assert s.profile_read()["k_convolve"]["launches"] == 2
    assert not s.get_frame_buffer().any()
    s.clear()
    s.convolve(CC.params(emboss, "clamp"))
    same(s.get_frame_buffer(), want, "a cleared scene in place under a bias")
    assert not clean_flags(s).any(), "a tile of 128s is flagged clean"
    assert s.profile_read()["k_convolve"]["launches"] == 3
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", [(640, 480), (134, 21)], ids=["whole_tile_rows", "partial_tile_row"])
def test_in_place_the_frame_and_its_flags_follow(small_synthetic, W, Hh):
    """The frame afterwards is the out-of-place result; resize, resolve and the sparse read-back see it; z stays; applied
    twice; a later clear and render is the caller's."""
    import tiny_renderer_amd as T
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    before = snap(s)
    fb = before["fb"]
    for name, edge, border in (("gaussian31", "border", (0, 0, 0)), ("emboss", "border", CC.PAPER), ("unsharp", "clamp", (0, 0, 0)), ("9x9_alternating", "clamp", (0, 0, 0))):
        case = ALL[name]
        want = host(fb, case, edge, border)
        assert not np.array_equal(want, fb)
        drive(s)
        assert s.convolve(CC.params(case, edge, border)) is None
        flags = clean_flags(s)
        lit = TR.lit_tiles(want, s.band_tiles())
        assert not (flags & lit).any(), "a tile that holds colour is flagged clean"
        if (W, Hh) == (640, 480) and name == "gaussian31":
            assert flags.any(), "after a blur under border 0 no tile is flagged clean"
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
        s.convolve(CC.params(case, edge, border))
        same(s.get_frame_buffer(), host(want, case, edge, border), name + ": twice")
    drive(s)
    TC.same(snap(s), before)
    s.close()


@pytest.mark.gpu
def test_a_convolve_between_two_renders_is_ordered_on_the_stream(small_synthetic):
    import torch
    W, Hh = 300, 200
    s = scene(W, Hh, small_synthetic, "phong", frames_per_launch=4)
    drive(s)
    fb = s.get_frame_buffer()
    a = torch.full((W * Hh * 3,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    TR.frame(s, CC.CAM, CC.LIGHT)
    s.convolve(CC.params(ALL["gaussian31"], "clamp"), a)
    TR.frame(s, 1.1, 0.2)
    assert s.sync() == 0
    two = s.get_frame_buffer()
    assert not np.array_equal(two, fb)
    same(a.cpu().numpy().reshape(Hh, W, 3), host(fb, ALL["gaussian31"], "clamp"), "the first frame, filtered before the second was rendered")
    s.close()


@pytest.mark.gpu
def test_no_depth_pass_is_provoked_and_the_profile_counts_the_launches(small_synthetic):
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong")
    s.profile_enable(True)
    drive(s)
    assert s.sync() == 0
    tiles = dict(s.profile_read())
    p = CC.params(ALL["3x7"])
    s.get_convolved(p)
    s.convolve(CC.params(ALL["tent7"], "clamp"), device_buffer(W * Hh * 3).data_ptr())
    s.convolve(p)
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_convolve", {}).get("launches") == 3 and prof["k_convolve"]["total_ms"] > 0.0, prof
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
    same(s.get_convolved(CC.params(ALL["unsharp"], "border", CC.PAPER)), host(fb, ALL["unsharp"], "border", CC.PAPER), pipe)
    s.close()


@pytest.mark.gpu
def test_the_device_tent_is_blooms_glow(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 640, 480
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    for R in (1, 3, 7, 15):
        k, shift = T.kernel_tent(R)
        same(s.get_convolved(T.convolve_params(k, shift=shift)), s.get_bloom(T.bloom_params(R, 0, 256, T.scene.BLOOM_GLOW_ONLY)), "radius %d" % R)
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
    p = CC.params(ALL["box3"])
    q = C.addressof(p)
    host_out = np.full((Hh, W, 3), 0xAA, np.uint8)
    dev = device_buffer(W * Hh * 3)
    text = lambda: L.tr_last_error().decode()
    calls = (("tr_scene_convolve", lambda sc, pp: L.tr_scene_convolve(sc._h, pp, dev.data_ptr())),
             ("tr_scene_get_convolved", lambda sc, pp: L.tr_scene_get_convolved(sc._h, pp, host_out.ctypes.data)))

    def wrong(**kw):
        w = CC.params(ALL["box3"])
        for k, v in kw.items():
            setattr(w, k, v)
        return w

    for who, call in calls:
        assert call(s, None) == _lib.TR_E_INVALID and text() == who + ": null argument"
        for kw, why in ((dict(struct_size=196), ": struct_size is not sizeof(tr_convolve_params)"), (dict(flags=8), ": unknown flags"),
                        (dict(kw=2), ": kw and kh must be odd and 1..9 (1..31 with TR_CONVOLVE_SEPARABLE)"),
                        (dict(kh=33, flags=1), ": kw and kh must be odd and 1..31 (TR_CONVOLVE_SEPARABLE)"),
                        (dict(shift=23), ": shift must be 0..22"), (dict(bias=-256), ": bias must be -255..255"),
                        (dict(amount=1025, flags=4), ": amount must be 0..1024"), (dict(amount=1), ": amount must be 0 without TR_CONVOLVE_UNSHARP"),
                        (dict(edge=2), ": edge must be TR_CONVOLVE_BORDER or TR_CONVOLVE_CLAMP"), (dict(pad=1), ": pad must be 0"),
                        (dict(flags=6), ": TR_CONVOLVE_UNSHARP does not go with TR_CONVOLVE_ABS"), (dict(flags=4, bias=1), ": TR_CONVOLVE_UNSHARP needs a bias of 0")):
            assert call(s, C.addressof(wrong(**kw))) == _lib.TR_E_INVALID and text() == who + why
        for kernel, why in CC.refused():
            bad = T.ConvolveParams(200, kernel[0].size, kernel[1].size, 1, 22, 0, 0, 0, (C.c_uint8 * 3)(), 0)
            for i, v in enumerate(np.concatenate(kernel)):
                bad.weights[i] = int(v)
            assert call(s, C.addressof(bad)) == _lib.TR_E_INVALID and text() == who + why
        # which refusal wins: the parameters before the band, the band before the target
        assert call(band, C.addressof(wrong(shift=23))) == _lib.TR_E_INVALID and text() == who + ": shift must be 0..22"
        assert call(band, q) == _lib.TR_E_INVALID
        assert text() == who + ": a band scene (tr_options.band_row0/1) cannot be convolved: its border taps lie in another rank's rows"
    assert L.tr_scene_convolve(None, q, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_convolve: null scene"
    assert L.tr_scene_get_convolved(None, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_convolved: null scene"
    assert L.tr_scene_get_convolved(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_convolved: null argument"
    assert L.tr_scene_convolve(band._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text().startswith("tr_scene_convolve: a band scene")
    with pytest.raises(T.TinyRendererError):
        band.get_convolved(p)
    assert L.tr_scene_convolve(s._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_convolve: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_convolved takes any host memory)"
    small = L.tr_host_alloc(W * Hh * 3 - 1)
    assert small
    assert L.tr_scene_convolve(s._h, q, small) == _lib.TR_E_INVALID and text() == "tr_scene_convolve: the host buffer is smaller than the frame"
    L.tr_host_free(small)
    t = s.band_tiles()
    assert L.tr_scene_convolve(s._h, q, int(t.frame_buffer_device) + 3) == _lib.TR_E_INVALID
    assert text() == "tr_scene_convolve: `out` overlaps a frame buffer of the scene (out == NULL convolves in place)"
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
    names = ("full", "blur", "sharp", "emboss", "edges", "custom", "small")
    full, blur, sharp, emboss, edges, custom, small = (str(tmp_path / (n + ".ppm")) for n in names)
    assert cli.main(common + ["--out", full]) == 0
    assert cli.main(common + ["--blur", "2.5", "--out", blur]) == 0
    assert cli.main(common + ["--sharpen", "1.5,2", "--out", sharp]) == 0
    assert cli.main(common + ["--emboss", "--out", emboss]) == 0
    assert cli.main(common + ["--edges", "--out", edges]) == 0
    assert cli.main(common + ["--convolve", "0,-1,0;-1,6,-1;0,-1,0", "--convolve-shift", "1", "--convolve-bias=-3", "--out", custom]) == 0
    assert cli.main(common + ["--blur", "2.5", "--out-size", "320x240", "--out", small]) == 0
    hd = b"P6\n640 480\n255\n"
    a, b, c, d, e, f = (np.frombuffer(open(p, "rb").read()[len(hd):], np.uint8).reshape(480, 640, 3) for p in (full, blur, sharp, emboss, edges, custom))
    assert a.any()
    g, gs = T.kernel_gaussian(2.5)
    blurred = T.convolve_host(a, T.convolve_params(g, shift=gs, edge="clamp"))
    same(b, blurred, "--blur")
    g2, g2s = T.kernel_gaussian(2.0)
    same(c, T.convolve_host(a, T.convolve_params(g2, shift=g2s, edge="clamp", unsharp=384)), "--sharpen")
    same(d, T.convolve_host(a, T.convolve_params(T.kernel_emboss()[0], bias=128, edge="clamp")), "--emboss")
    same(e, T.convolve_host(a, T.convolve_params(T.kernel_laplacian()[0], edge="clamp", absolute=True)), "--edges")
    same(f, T.convolve_host(a, T.convolve_params(np.array([[0, -1, 0], [-1, 6, -1], [0, -1, 0]], np.int32), shift=1, bias=-3)), "--convolve")
    hs = b"P6\n320 240\n255\n"
    h = np.frombuffer(open(small, "rb").read()[len(hs):], np.uint8).reshape(240, 320, 3)
    same(h, T.resize_host(blurred, 320, 240), "--blur before --out-size")
    for bad in (["--blur", "2", "--view", "z"], ["--sharpen", "x"], ["--convolve", "1,2;3"], ["--convolve", "1,2;3,4"], ["--convolve-shift", "2"], ["--blur", "2", "--convolve-shift", "3"], ["--emboss", "--convolve-bias", "3"],
                ["--blur", "2", "--seconds", "1"], ["--convolve", "1", "--convolve-shift", "23"]):
        with pytest.raises(SystemExit):
            cli.main(common + bad)
