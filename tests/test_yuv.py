"""YUV output on the device: tr_scene_to_yuv / tr_scene_to_yuv_from / tr_scene_get_yuv (k_yuv) equal tr_yuv_host in every
byte.

Every comparison is np.array_equal against yuv_host of the frame the scene itself returns; tests/test_yuv_host.py pins
yuv_host against the rule in numpy and the tables against their derivation.  The sizes are tests/yuv_cases.py's: units of
eight columns with flagged and unflagged tiles (640 x 480), units of four and an odd height (132 x 17), bytes and
unaligned chroma planes (131 x 19), a partial tile column and top tile row (1000 x 488), one unit (8 x 8), one pixel."""
import ctypes as C

import numpy as np
import pytest

from tests import test_composite as TC
from tests import test_outline as TO
from tests import test_resolve as TR
from tests import yuv_cases as YC

scene, snap, clean_flags = TC.scene, TC.snap, TC.clean_flags
other_synthetic = TC.other_synthetic
device_buffer = TO.device_buffer
PIPELINES = TR.PIPELINES
GUARD = 64
ONE = ("i420", "bt709", "limited")


def drive(s, cam=YC.CAM, light=YC.LIGHT, clear=True):
    TC.drive(s, cam, light, clear)


def host(fb, layout="i420", matrix="bt709", rng="limited"):
    import tiny_renderer_amd as T
    return T.yuv_host(fb, layout, matrix, rng, flat=True)


def flat(planes):
    return np.concatenate([p.reshape(-1) for p in planes])


def same(got, want, what):
    got, want = (flat(v) if isinstance(v, tuple) else np.asarray(v).reshape(-1) for v in (got, want))
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d bytes differ" % (what, int((got != want).sum()))


def every(s, fb, what, combos=None):
    for layout, matrix, rng in combos or [(l, m, r) for l in YC.LAYOUTS for m, r in YC.TABLES]:
        same(s.to_yuv(layout, matrix, rng), host(fb, layout, matrix, rng), "%s %s %s %s" % (what, layout, matrix, rng))


@pytest.mark.gpu
@pytest.mark.parametrize("W,Hh", YC.GPU_ALL + YC.GPU_ONE, ids=["%dx%d" % s for s in YC.GPU_ALL + YC.GPU_ONE])
def test_planes_equal_the_host_rule(small_synthetic, W, Hh):
    s = scene(W, Hh, small_synthetic, "phong") if (W, Hh) != (1, 1) else None
    if s is None:
        # (tr_scene_create's smallest frame is 8 x 8: one pixel goes through tr_scene_to_yuv_from)
        import torch
        s = scene(8, 8, small_synthetic, "phong")
        for colour in ((0, 0, 255), (255, 0, 0), (17, 130, 240)):
            px = torch.tensor(colour, dtype=torch.uint8, device="cuda").reshape(1, 1, 3)
            torch.cuda.synchronize()
            for layout in YC.LAYOUTS:
                for matrix, rng in YC.TABLES:
                    same(s.to_yuv_from(px, layout, matrix, rng), host(px.cpu().numpy(), layout, matrix, rng), "1x1 %r" % (colour,))
        s.close()
        return
    drive(s)
    fb = s.get_frame_buffer()
    assert fb.any() and not fb.all(-1).all()
    if (W, Hh) == (640, 480):
        flags = clean_flags(s)
        assert flags.any() and not flags.all(), "640 x 480 holds flagged and unflagged tiles"
    every(s, fb, "%dx%d" % (W, Hh), None if (W, Hh) in YC.GPU_ALL else [ONE, ("nv12", "bt601", "full"), ("i444", "bt601", "limited")])
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", PIPELINES)
def test_every_pipeline(small_synthetic, pipe):
    s = scene(640, 480, small_synthetic, pipe)
    drive(s)
    fb = s.get_frame_buffer()
    drive(s)
    same(s.to_yuv(*ONE), host(fb, *ONE), pipe)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", YC.LAYOUTS)
@pytest.mark.parametrize("W,Hh", [(640, 480), (132, 17), (131, 19)], ids=["units-of-8", "units-of-4", "bytes"])
def test_device_pinned_and_getter_targets_between_guards(small_synthetic, W, Hh, layout):
    """A torch tensor, a tr_host_alloc block and the getter, each pre-filled with 0xAA between guard bytes: every byte
    inside is written, none outside.  A device pointer off by one byte takes the byte form and gives the same planes."""
    import torch
    import tiny_renderer_amd as T
    s = scene(W, Hh, small_synthetic, "specular")
    drive(s)
    want = host(s.get_frame_buffer(), layout, "bt601", "full")
    n = want.size
    assert n == T.yuv_bytes(W, Hh, layout) and want.any() and not (want == 0xAA).all()
    dev = torch.full((n + 2 * GUARD,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    for off in (0, 1):
        dev[:] = 0xAA
        torch.cuda.synchronize()
        drive(s)
        s.to_yuv_into(dev.data_ptr() + GUARD + off, layout, "bt601", "full")
        assert s.sync() == 0
        raw = dev.cpu().numpy()
        same(raw[GUARD + off:GUARD + off + n], want, "device + %d" % off)
        assert (raw[:GUARD + off] == 0xAA).all() and (raw[GUARD + off + n:] == 0xAA).all(), "a guard byte changed"
    whole = torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda")
    assert s.to_yuv_into(whole, layout, "bt601", "full") is whole
    assert s.sync() == 0
    same(whole.cpu().numpy(), want, "tensor")
    L = T.load_library()
    block = L.tr_host_alloc(n + 2 * GUARD)
    assert block
    pinned = np.ctypeslib.as_array((C.c_uint8 * (n + 2 * GUARD)).from_address(block))
    pinned[:] = 0xAA
    p = T.yuv_params(layout, "bt601", "full")
    assert L.tr_scene_to_yuv(s._h, C.addressof(p), block) == 0 and s.sync() == 0
    same(pinned[:n], want, "tr_host_alloc block")
    assert (pinned[n:] == 0xAA).all(), "bytes behind the planes changed"
    L.tr_host_free(block)
    mine = s.pinned_yuv(layout)
    mine[...] = 0xAA
    assert s.to_yuv_into(mine, layout, "bt601", "full") is mine and s.sync() == 0
    same(mine, want, "pinned_yuv")
    for off in (0, 1):
        guarded = np.full(n + 2 * GUARD + 1, 0xAA, np.uint8)
        assert L.tr_scene_get_yuv(s._h, C.addressof(p), guarded[GUARD + off:].ctypes.data) == 0
        same(guarded[GUARD + off:GUARD + off + n], want, "getter + %d" % off)
        assert (guarded[:GUARD + off] == 0xAA).all() and (guarded[GUARD + off + n:] == 0xAA).all()
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["noise", "white"])
def test_a_dense_frame_with_planted_blue_and_red_blocks(small_synthetic, kind):
    """tests/dense_cases.py's frames: a caller's buffer of noise (or white) drawn into without a clear, with pure blue and
    pure red 2 x 2 blocks planted where nothing is drawn.  No tile is flagged, every byte value occurs and the clamp acts."""
    import torch
    from tests import dense_cases as DC
    from tests import test_dense_frames as TD
    for W, Hh in DC.SIZES:
        s, buf, f = TD.dense_scene(small_synthetic, W, Hh, kind)
        assert s.sync() == 0
        view = buf[DC.GUARD:DC.GUARD + W * Hh * 3].view(Hh, W, 3)
        drawn = (DC.bits(f["z"]) != DC.F32_MIN_BITS)[::-1]
        # two aligned 2 x 2 blocks in the bottom row of blocks, where the model is not
        y, xb, xr = (Hh - 2) // 2 * 2 - 2, 0, 2 * ((W - 2) // 2)
        assert not drawn[y:y + 2, xb:xb + 2].any() and not drawn[y:y + 2, xr:xr + 2].any()
        view[y:y + 2, xb:xb + 2] = torch.tensor([0, 0, 255], dtype=torch.uint8, device="cuda")
        view[y:y + 2, xr:xr + 2] = torch.tensor([255, 0, 0], dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fb = s.get_frame_buffer()
        assert (fb[y:y + 2, xb:xb + 2] == (0, 0, 255)).all() and (fb[y:y + 2, xr:xr + 2] == (255, 0, 0)).all()
        if kind == "noise":
            assert len(np.unique(fb)) == 256
        raw = YC.rule_np(fb, "i420", "bt601", "full", raw=True)
        assert raw[1][y // 2, xb // 2] == 256 and raw[2][y // 2, xr // 2] == 256, "the clamp acts on the planted blocks"
        every(s, fb, "%s %dx%d" % (kind, W, Hh))
        got = s.to_yuv("i420", "bt601", "full")
        assert got[1][y // 2, xb // 2] == 255 and got[2][y // 2, xr // 2] == 255
        TD.in_buffer(buf, fb)
        s.close()


@pytest.mark.gpu
def test_an_odd_height_pairs_a_flagged_tile_row_with_an_unflagged_one(small_synthetic):
    """H = 479: every border between two tile rows falls between the two rows of a chroma pair.  A frame that covers
    the screen, then a clear and the small model: tiles lit in the first frame and flagged clean in the second count as
    zeros -- also in the pairs they share with an unflagged tile -- whatever their memory holds.  Then the cleared scene."""
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = 640, 479
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
    stale = lit_one & ~flags_one & flags_two
    assert stale.any(), "no tile lit in frame one is flagged clean in frame two"
    # a flagged tile with stale colour right above or below an unflagged one: they share the chroma row at their border
    pairs = (stale[1:] & ~flags_two[:-1]) | (stale[:-1] & ~flags_two[1:])
    assert pairs.any(), "no flagged tile row meets an unflagged one"
    # ... and the flagged tile's row of such a pair held colour in frame one: read from memory, it would show in the pair
    up = one[::-1]
    stale_border = False
    for ty, tx in zip(*np.nonzero(stale[1:] & ~flags_two[:-1])):     # flagged above (ty + 1), unflagged below (ty)
        stale_border = stale_border or up[16 * ty + 16, 128 * tx:128 * tx + 128].any()
    for ty, tx in zip(*np.nonzero(stale[:-1] & ~flags_two[1:])):     # flagged below (ty), unflagged above (ty + 1)
        stale_border = stale_border or up[16 * ty + 15, 128 * tx:128 * tx + 128].any()
    assert stale_border, "no flagged border row held colour before"
    every(s, two, "odd height")
    s.profile_enable(True)
    s.clear()
    for layout in YC.LAYOUTS:
        n = T.yuv_bytes(W, Hh, layout)
        dev = device_buffer(n)
        s.to_yuv_into(dev.data_ptr(), layout, "bt709", "limited")
        assert s.sync() == 0
        black = host(np.zeros((Hh, W, 3), np.uint8), layout)
        assert set(np.unique(black)) == {16, 128}
        same(dev.cpu().numpy(), black, "a cleared scene gives the planes of black")
        s.clear()
        same(s.to_yuv(layout, "bt601", "full"), host(np.zeros((Hh, W, 3), np.uint8), layout, "bt601", "full"), "the getter on a cleared scene")
    assert "k_yuv" not in s.profile_read(), "a cleared scene launches nothing"
    s.close()


@pytest.mark.gpu
def test_ordering_and_kept_frames(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    mesh, texs = small_synthetic
    W, Hh = 300, 200
    s = T.Scene(W, Hh, mesh, texs, "phong", frames_per_launch=4)
    n = T.yuv_bytes(W, Hh, "i420")
    a, b = (torch.full((n,), 0xAA, dtype=torch.uint8, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    TR.frame(s, 0.3, 0.7)          # may be held back on the host: no getter follows
    s.to_yuv_into(a)
    TR.frame(s, 1.1, 0.2)          # overwrites the frame the conversion reads: must run after it
    s.to_yuv_into(b, "i420", "bt601", "full")
    assert s.sync() == 0
    two = s.get_frame_buffer()
    TR.frame(s, 0.3, 0.7)
    one = s.get_frame_buffer()
    assert not np.array_equal(one, two)
    same(a.cpu().numpy(), host(one), "the first frame, converted before the second was rendered")
    same(b.cpu().numpy(), host(two, "i420", "bt601", "full"), "the second frame")
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
        same(s.to_yuv("nv12"), host(frames[back], "nv12"), "kept frame %d" % back)
    s.close()


@pytest.mark.gpu
def test_after_composite_grade_and_convolve_in_place(small_synthetic, other_synthetic):
    import tiny_renderer_amd as T
    from tests import test_grade as TG
    W, Hh = 300, 200
    s = scene(W, Hh, small_synthetic, "phong", TC.DST_AT)
    o = scene(W, Hh, other_synthetic, "phong", TC.SRC_AT)
    drive(s), drive(o)
    alone = s.get_frame_buffer()
    s.composite(o)
    merged = s.get_frame_buffer()
    assert not np.array_equal(alone, merged)
    same(s.to_yuv(*ONE), host(merged, *ONE), "after composite")
    lut = TG.random_lut(17, 5)
    graded = T.grade_host(merged, lut)
    s.set_lut(lut), s.grade()
    same(s.to_yuv("i444", "bt601", "full"), host(graded, "i444", "bt601", "full"), "after grade in place")
    g, gs = T.kernel_gaussian(1.5)
    cp = T.convolve_params(g, shift=gs, edge="clamp")
    blurred = T.convolve_host(graded, cp)
    assert not np.array_equal(blurred, graded)
    s.convolve(cp)
    same(s.get_frame_buffer(), blurred, "convolve in place")
    same(s.to_yuv("nv12", "bt709", "full"), host(blurred, "nv12", "bt709", "full"), "after convolve in place")
    s.close(), o.close()


@pytest.mark.gpu
def test_to_yuv_from_takes_the_outputs_of_resize_resolve_and_warp(small_synthetic):
    import torch
    import tiny_renderer_amd as T
    W, Hh = 300, 200
    s = scene(W, Hh, small_synthetic, "phong")
    drive(s)
    fb = s.get_frame_buffer()
    # resize to an odd size, resolve by 2, each into a device tensor, converted behind it without a wait
    small = torch.full((97, 211, 3), 0xAA, dtype=torch.uint8, device="cuda")
    half = torch.full((Hh // 2, W // 2, 3), 0xAA, dtype=torch.uint8, device="cuda")
    outs = {k: torch.full((T.yuv_bytes(w, h, "i420"),), 0xAA, dtype=torch.uint8, device="cuda") for k, (w, h) in (("small", (211, 97)), ("half", (W // 2, Hh // 2)))}
    torch.cuda.synchronize()
    s.resize_into(small, 211, 97)
    assert s.to_yuv_from(small, target=outs["small"]) is outs["small"]
    s.resolve_into(2, half.data_ptr())
    s.to_yuv_from(half.data_ptr(), "i420", "bt601", "full", target=outs["half"], width=W // 2, height=Hh // 2)
    assert s.sync() == 0
    same(small.cpu().numpy(), T.resize_host(fb, 211, 97), "the resized image")
    same(outs["small"].cpu().numpy(), host(T.resize_host(fb, 211, 97)), "planes of the resized image")
    same(outs["half"].cpu().numpy(), host(TR.box(fb, 2), "i420", "bt601", "full"), "planes of the resolved image")
    # ... and the synchronous form, every layout, from a page-locked image too
    for layout in YC.LAYOUTS:
        same(s.to_yuv_from(small, layout), host(T.resize_host(fb, 211, 97), layout), "to_yuv_from " + layout)
    pinned = s.pinned_resized(211, 97)
    s.resize_into(pinned, 211, 97)
    same(s.to_yuv_from(pinned, "nv12"), host(T.resize_host(fb, 211, 97), "nv12"), "from a page-locked image")
    # warp: out of place into a tensor of the frame's size
    warped = torch.full((Hh, W, 3), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    grid = T.warp_grid_rotate(10.0, W, Hh)
    wp = T.warp_params()
    s.set_warp(grid, W, Hh)
    s.warp(wp, out=warped)
    got = s.to_yuv_from(warped, "i444")
    rotated = T.warp_host(fb, grid, W, Hh, wp)
    assert not np.array_equal(rotated, fb)
    same(warped.cpu().numpy(), rotated, "the warped image")
    same(got, host(rotated, "i444"), "planes of the warped image")
    # refusals of this entry point
    L = T.load_library()
    from tiny_renderer_amd import _lib
    text = lambda: L.tr_last_error().decode()
    p = T.yuv_params()
    q = C.addressof(p)
    n = T.yuv_bytes(211, 97, "i420")
    both = torch.full((211 * 97 * 3 + n,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert L.tr_scene_to_yuv_from(s._h, both.data_ptr(), 211, 97, q, both.data_ptr() + 211 * 97 * 3 - 1) == _lib.TR_E_INVALID
    assert text() == "tr_scene_to_yuv_from: `rgb` overlaps `out` (there is no in-place form)"
    assert L.tr_scene_to_yuv_from(s._h, both.data_ptr(), 211, 97, q, both.data_ptr() + 211 * 97 * 3) == 0 and s.sync() == 0
    ordinary = np.zeros((97, 211, 3), np.uint8)
    assert L.tr_scene_to_yuv_from(s._h, ordinary.ctypes.data, 211, 97, q, outs["small"].data_ptr()) == _lib.TR_E_INVALID
    assert text() == "tr_scene_to_yuv_from: `rgb` is neither device memory nor from tr_host_alloc (tr_yuv_host takes any host memory)"
    for w, h in ((0, 97), (211, 8193)):
        assert L.tr_scene_to_yuv_from(s._h, both.data_ptr(), w, h, q, outs["small"].data_ptr()) == _lib.TR_E_INVALID
        assert text() == "tr_scene_to_yuv_from: width and height must be 1..8192"
    assert L.tr_scene_to_yuv_from(s._h, None, 211, 97, q, outs["small"].data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_to_yuv_from: null argument"
    assert L.tr_scene_to_yuv_from(s._h, both.data_ptr(), 211, 97, q, None) == _lib.TR_E_INVALID
    s.close()


@pytest.mark.gpu
def test_no_depth_pass_is_provoked_and_the_profile_counts_the_launches(small_synthetic):
    import tiny_renderer_amd as T
    W, Hh = 256, 48
    s = scene(W, Hh, small_synthetic, "phong")     # (depth is transient by default: a depth pass would show as k_tile_depth)
    s.profile_enable(True)
    drive(s)
    assert s.sync() == 0
    tiles = dict(s.profile_read())
    s.to_yuv()
    s.to_yuv_into(device_buffer(T.yuv_bytes(W, Hh, "i444")).data_ptr(), "i444")
    assert s.sync() == 0
    prof = s.profile_read()
    assert prof.get("k_yuv", {}).get("launches") == 2 and prof["k_yuv"]["total_ms"] > 0.0, prof
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
    p = T.yuv_params()
    q = C.addressof(p)
    n = T.yuv_bytes(W, Hh, "i420")
    host_out = np.full(n, 0xAA, np.uint8)
    dev = device_buffer(n)
    s.profile_enable(True), band.profile_enable(True)
    text = lambda: L.tr_last_error().decode()
    band_text = (": a band scene (tr_options.band_row0/1) cannot be converted: a chroma sample's pair of rows straddles a band's border, "
                 "and its planes are not the frame's rows")
    assert L.tr_scene_to_yuv(band._h, q, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_to_yuv" + band_text
    assert L.tr_scene_get_yuv(band._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_yuv" + band_text
    with pytest.raises(T.TinyRendererError):
        band.to_yuv()
    assert L.tr_scene_to_yuv(s._h, q, None) == _lib.TR_E_INVALID
    assert text() == "tr_scene_to_yuv: out == NULL (the planes are no frame of the scene: there is no in-place form)"
    with pytest.raises(ValueError):
        s.to_yuv_into(None)
    assert L.tr_scene_to_yuv(s._h, None, dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_to_yuv: null argument"
    assert L.tr_scene_get_yuv(s._h, q, None) == _lib.TR_E_INVALID and text() == "tr_scene_get_yuv: null argument"
    for fields, why in (((3, 0, 0, 0), ": layout must be TR_YUV_I420, TR_YUV_NV12 or TR_YUV_I444"), ((0, 2, 0, 0), ": matrix must be TR_YUV_BT601 or TR_YUV_BT709"),
                        ((0, 0, 2, 0), ": range must be TR_YUV_FULL or TR_YUV_LIMITED"), ((0, 0, 0, 4), ": flags must be 0")):
        bad = T.YuvParams(*fields)
        assert L.tr_scene_to_yuv(s._h, C.addressof(bad), dev.data_ptr()) == _lib.TR_E_INVALID and text() == "tr_scene_to_yuv" + why
        assert L.tr_scene_get_yuv(s._h, C.addressof(bad), host_out.ctypes.data) == _lib.TR_E_INVALID and text() == "tr_scene_get_yuv" + why
        assert L.tr_scene_to_yuv_from(s._h, dev.data_ptr(), 8, 8, C.addressof(bad), dev.data_ptr() + 4096) == _lib.TR_E_INVALID and text() == "tr_scene_to_yuv_from" + why
    assert L.tr_scene_to_yuv(s._h, q, host_out.ctypes.data) == _lib.TR_E_INVALID
    assert text() == "tr_scene_to_yuv: `out` is neither device memory nor from tr_host_alloc (tr_scene_get_yuv takes any host memory)"
    small = L.tr_host_alloc(n - 1)
    assert small
    assert L.tr_scene_to_yuv(s._h, q, small) == _lib.TR_E_INVALID and text() == "tr_scene_to_yuv: the host buffer is smaller than the planes"
    L.tr_host_free(small)
    assert L.tr_scene_to_yuv(s._h, q, s.frame_buffer_device()) == _lib.TR_E_INVALID
    assert text() == "tr_scene_to_yuv: `out` overlaps a frame buffer of the scene (there is no in-place form)"
    assert (host_out == 0xAA).all() and (dev.cpu().numpy() == 0x5A).all(), "a refused call wrote `out`"
    for q_, f_, fl_, rows in ((s, before, flags, None), (band, before_band, flags_band, (16, 32))):
        assert q_.sync() == 0
        assert "k_yuv" not in q_.profile_read(), "a refused call queued a kernel"
        assert np.array_equal(clean_flags(q_), fl_)
        TC.same(snap(q_), f_, rows)
    s.close(), band.close()


@pytest.mark.gpu
def test_cli_writes_every_frame_of_a_run_to_a_y4m_file(built, tmp_path):
    import tiny_renderer_amd as T
    from tiny_renderer_amd import cli
    W, Hh, n = 132, 17, 3
    path = str(tmp_path / "x.y4m")
    assert cli.main(["--synthetic", "-s", "phong", "--width", str(W), "--height", str(Hh), "--frames", str(n), "--fps", "24", "--out", path]) == 0
    fields, frames = YC.parse_y4m(path)
    assert fields == ["YUV4MPEG2", "W%d" % W, "H%d" % Hh, "F24:1", "Ip", "A1:1", "C420jpeg", "XCOLORRANGE=LIMITED"] and len(frames) == n
    mesh, texs = T.synthetic_scene()     # (what --synthetic builds)
    s = T.Scene(W, Hh, mesh, texs, "phong")
    seen = []
    for f in range(n):
        ca, la = np.float32(0.0 + 2.0 * np.pi * f / n), np.float32(0.0)
        s.clear()
        s.set_light_direction([float(np.sin(la)), 0.0, float(np.cos(la))])
        s.set_camera([float(np.sin(ca)), 0.0, float(np.cos(ca))], [0, 0, 0], [0, 1, 0])
        s.render()
        fb = s.get_frame_buffer()
        assert fb.any()
        seen.append(fb)
        same(frames[f], host(fb), "frame %d of the file" % f)
    assert not np.array_equal(seen[0], seen[1])
    # resized on the device first, 4:4:4, full range
    assert cli.main(["--synthetic", "-s", "phong", "--width", str(W), "--height", str(Hh), "--frames", "2", "--out-size", "67x9",
                     "--yuv-layout", "i444", "--yuv-range", "full", "--yuv-matrix", "bt601", "--out", path]) == 0
    fields, frames = YC.parse_y4m(path)
    assert fields[1:3] == ["W67", "H9"] and fields[6:] == ["C444", "XCOLORRANGE=FULL"] and len(frames) == 2
    s.clear()
    s.set_light_direction([0.0, 0.0, 1.0]), s.set_camera([0.0, 0.0, 1.0], [0, 0, 0], [0, 1, 0]), s.render()
    same(frames[0], host(T.resize_host(s.get_frame_buffer(), 67, 9), "i444", "bt601", "full"), "--out-size before the planes")
    for bad in (["--shutter", "2"], ["--view", "z"], ["--fps", "0"]):
        with pytest.raises(SystemExit):
            cli.main(["--synthetic", "--frames", "3", "--out", path] + bad)
    s.close()

